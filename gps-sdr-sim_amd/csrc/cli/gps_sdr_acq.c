/*
 * gps-sdr-acq — the acquisition search (include/gpssim_amd.h, gss_acquire_*) over a file of I/Q
 * samples as gps-sdr-sim writes them: are the satellites there, at which code phase and Doppler,
 * and at what level.  One line per PRN: PRN found tau_samples doppler_hz ratio cn0_dbhz.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gpssim_amd.h"
#include "cli_rx.h"

static void usage(void)
{
    fprintf(stderr,
        "Usage: gps-sdr-acq [options]\n"
        "Options:\n"
        "  -f <file>        I/Q sample file (required)\n"
        "  -s <frequency>   Sampling frequency [Hz] (required)\n"
        "  -b <iq_bits>     I/Q data format [1/8/16] (default: 16)\n"
        "  -t <seconds>     Start of the search in the file (default: 0)\n"
        "  --coh-ms=<ms>    Coherent window (default: 1)\n"
        "  --ncoh=<M>       Windows summed non-coherently (default: 10)\n"
        "  --fmax=<Hz>      Doppler search range +- (default: 10000)\n"
        "  --bin-hz=<Hz>    Doppler bin width (default: 500 / coh-ms)\n"
        "  --prn=<list>     PRNs, e.g. 1,3,7-9 (default: 1-32)\n"
        "  --pfa=<p>        False-alarm probability of the search (default: 1e-3)\n"
        "  --qshift=<s>     Quantiser shift 0..24 (default: auto)\n"
        "  --host           Search on the CPU (no GPU needed)\n"
        "  --grid=<file>    Write the power grid [PRN][bin][tau] as uint64\n");
}

static int parse_long(const char *s, long lo, long hi, long *out)
{
    char *end;
    if (!*s)
        return -1;
    const long v = strtol(s, &end, 10);
    if (*end || v < lo || v > hi)
        return -1;
    *out = v;
    return 0;
}

int main(int argc, char **argv)
{
    const char *grid_file = NULL;
    rx_opts_t o = RX_OPTS_DEFAULT;
    double pfa = 1e-3;
    long coh = 1, ncoh = 10, fmax = 10000, bin_hz = 0, qshift = -1;
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
        if (!strncmp(a, "--coh-ms=", 9)) {
            if (parse_long(a + 9, 1, 1000000, &coh))
                return rx_fail("Invalid coherent window.");
        } else if (!strncmp(a, "--ncoh=", 7)) {
            if (parse_long(a + 7, 1, 1000, &ncoh))
                return rx_fail("Invalid number of windows (1..1000).");
        } else if (!strncmp(a, "--fmax=", 7)) {
            if (parse_long(a + 7, 0, 1000000000, &fmax))
                return rx_fail("Invalid Doppler range.");
        } else if (!strncmp(a, "--bin-hz=", 9)) {
            if (parse_long(a + 9, 1, 1000000000, &bin_hz))
                return rx_fail("Invalid Doppler bin width.");
        } else if (!strncmp(a, "--prn=", 6)) {
            if (rx_parse_prns(a + 6, &mask))
                return rx_fail("Invalid PRN list (1..32, e.g. 1,3,7-9).");
        } else if (!strncmp(a, "--pfa=", 6)) {
            pfa = strtod(a + 6, &end);
            if (*end || !(pfa > 0.0) || !(pfa < 1.0))
                return rx_fail("Invalid false-alarm probability.");
        } else if (!strncmp(a, "--qshift=", 9)) {
            if (parse_long(a + 9, 0, 24, &qshift))
                return rx_fail("Invalid quantiser shift (0..24).");
        } else if (!strcmp(a, "--host")) {
            host = 1;
        } else if (!strncmp(a, "--grid=", 7)) {
            grid_file = a + 7;
        } else {
            usage();
            return 1;
        }
    }
    if (rx_required(&o))
        return 1;
    const double fs = o.fs;
    const long bits = o.bits;
    if (bin_hz == 0)
        bin_hz = coh <= 500 ? 500 / coh : 1;

    gss_acq_t acq;
    acq.fs_hz = (int32_t)fs;
    acq.fmt = (int32_t)bits;
    acq.coh_ms = (int32_t)coh;
    acq.n_coh = (int32_t)ncoh;
    acq.bin_hz = (int32_t)bin_hz;
    acq.n_half = (int32_t)(fmax / bin_hz);
    acq.qshift = (int32_t)qshift;
    acq.prn_mask = mask;
    int32_t T, n_prn;
    int64_t N;
    if (gss_acq_sizes(&acq, NULL, &T, &N, NULL, &n_prn)) {
        fprintf(stderr, "ERROR: %s\n", gss_last_error());
        return 1;
    }
    if (gss_last_error()[0])
        fprintf(stderr, "%s\n", gss_last_error());

    const int64_t first = rx_first_sample(&o);
    FILE *fp = fopen(o.file, "rb");
    if (!fp)
        return rx_fail("Failed to open the sample file.");
    void *x = malloc(rx_bytes(bits, N));
    const size_t nbin = (size_t)(2 * acq.n_half + 1);
    gss_acq_peak_t *peaks = (gss_acq_peak_t *)calloc((size_t)n_prn, sizeof *peaks);
    uint64_t *grid = grid_file ? (uint64_t *)malloc((size_t)n_prn * nbin * T * 8) : NULL;
    if (!x || !peaks || (grid_file && !grid))
        return rx_fail("Out of memory.");
    if (rx_read(fp, bits, first, N, x)) {
        fclose(fp);
        return rx_fail("The sample file is too short for this search.");
    }
    fclose(fp);

    int sh = 0, rc;
    if (host) {
        rc = gss_acquire_host(&acq, x, peaks, grid, &sh, 8);
    } else {
        gss_dev *dev = NULL;
        rc = gss_dev_open(&dev, 0);
        if (rc == 0) {
            rc = gss_acquire(dev, &acq, x, peaks, grid, &sh);
            gss_dev_close(dev);
        }
    }
    if (rc) {
        fprintf(stderr, "ERROR: %s\n", gss_last_error());
        return 1;
    }
    const double thr = gss_acq_threshold(acq.n_coh, (uint64_t)nbin * (uint64_t)T, pfa);
    fprintf(stderr, "Search: %lld samples from %lld, %zu bins of %d Hz, shift = %d, "
            "threshold = %.4f\n", (long long)N, (long long)first, nbin, acq.bin_hz, sh, thr);
    for (int p = 0; p < n_prn; p++) {
        const double ratio = rx_peak_ratio(&peaks[p]);
        const double cn0 = ratio > 1.0 ? 10.0 * log10((ratio - 1.0) / (acq.coh_ms * 1e-3))
                                       : -INFINITY;
        printf("%2d %d %d %d %.6f %.3f\n", peaks[p].prn, ratio >= thr, peaks[p].tau,
               peaks[p].bin * acq.bin_hz, ratio, cn0);
    }
    if (grid_file) {
        FILE *g = fopen(grid_file, "wb");
        const size_t cells = (size_t)n_prn * nbin * T;
        if (!g || fwrite(grid, 8, cells, g) != cells)
            return rx_fail("Failed to write the grid file.");
        fclose(g);
    }
    free(x);
    free(peaks);
    free(grid);
    return 0;
}
