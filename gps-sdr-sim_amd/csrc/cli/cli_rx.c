/* cli_rx.c — shared by gps-sdr-acq and gps-sdr-track (cli_rx.h); linked into the tools only */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "cli_rx.h"

int rx_fail(const char *msg)
{
    fprintf(stderr, "ERROR: %s\n", msg);
    return 1;
}

int rx_option(int argc, char **argv, int *i, rx_opts_t *o, void (*usage)(void))
{
    const char *a = argv[*i];
    char *end;
    if (strcmp(a, "-f") && strcmp(a, "-s") && strcmp(a, "-b") && strcmp(a, "-t"))
        return 0;
    if (*i + 1 >= argc) {
        usage();
        return -1;
    }
    const char *v = argv[++*i];
    const char *bad = NULL;
    if (a[1] == 'f') {
        o->file = v;
    } else if (a[1] == 's') {
        o->fs = strtod(v, &end);
        if (*end || !(o->fs >= 1000.0) || o->fs > 2e9 || o->fs != floor(o->fs))
            bad = "Invalid sampling frequency.";
    } else if (a[1] == 'b') {
        o->bits = strtol(v, &end, 10);
        if (*end || (o->bits != 1 && o->bits != 8 && o->bits != 16))
            bad = "Invalid I/Q data format.";
    } else {
        o->t0 = strtod(v, &end);
        if (*end || !(o->t0 >= 0.0))
            bad = "Invalid start time.";
    }
    return bad ? -rx_fail(bad) : 1;
}

int rx_required(const rx_opts_t *o)
{
    if (!o->file)
        return rx_fail("Sample file is not specified.");
    if (o->fs == 0)
        return rx_fail("Sampling frequency is not specified.");
    return 0;
}

int rx_parse_prns(const char *s, uint32_t *mask)
{
    *mask = 0;
    while (*s) {
        char *end;
        long a = strtol(s, &end, 10), b;
        if (end == s)
            return -1;
        b = a;
        if (*end == '-') {
            s = end + 1;
            b = strtol(s, &end, 10);
            if (end == s)
                return -1;
        }
        if (a < 1 || b > 32 || a > b)
            return -1;
        for (long p = a; p <= b; p++)
            *mask |= 1u << (p - 1);
        if (*end == ',')
            end++;
        else if (*end)
            return -1;
        s = end;
    }
    return *mask ? 0 : -1;
}

size_t rx_bytes(long bits, int64_t n)
{
    return bits == 16 ? (size_t)n * 4 : bits == 8 ? (size_t)n * 2 : (size_t)(n + 3) / 4;
}

int64_t rx_offset(long bits, int64_t first)
{
    return bits == 16 ? first * 4 : bits == 8 ? first * 2 : first / 4;
}

int64_t rx_first_sample(const rx_opts_t *o)
{
    int64_t first = (int64_t)floor(o->t0 * o->fs);
    if (o->bits == 1)
        first -= first % 4;
    return first;
}

int rx_read(FILE *fp, long bits, int64_t first, int64_t n, void *x)
{
    const size_t nb = rx_bytes(bits, n);
    return fseeko(fp, (off_t)rx_offset(bits, first), SEEK_SET) != 0 || fread(x, 1, nb, fp) != nb
               ? -1 : 0;
}

double rx_peak_ratio(const gss_acq_peak_t *p)
{
    return p->floor_sum ? (double)p->peak * (double)p->floor_cnt / (double)p->floor_sum : 0.0;
}
