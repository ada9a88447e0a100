/* cli_rx.h — what the receiver-side tools (gps-sdr-acq, gps-sdr-track) share: the options that
   name the sample file and its format, the PRN list, and reading a range of samples. */
#ifndef CLI_RX_H
#define CLI_RX_H

#include <stdint.h>
#include <stdio.h>
#include "gpssim_amd.h"

typedef struct rx_opts {
    const char *file;                /* -f */
    double fs, t0;                   /* -s, -t */
    long bits;                       /* -b */
} rx_opts_t;

#define RX_OPTS_DEFAULT {NULL, 0, 0, 16}

/* "ERROR: msg" on stderr; returns 1, the tools' exit status */
int rx_fail(const char *msg);
/* argv[*i] as one of -f -s -b -t: 0 when it is none of them, 1 when taken (*i then stands on its
   value), -1 when the tool ends with status 1: the value is missing (the tool's usage text has
   been printed) or invalid (reported) */
int rx_option(int argc, char **argv, int *i, rx_opts_t *o, void (*usage)(void));
/* after the options: 0, or 1 with the message when -f or -s is missing */
int rx_required(const rx_opts_t *o);
/* a PRN list such as 1,3,7-9 into a mask (bit p - 1); -1 when invalid or empty */
int rx_parse_prns(const char *s, uint32_t *mask);
/* the bytes of n samples, and the byte at which sample `first` starts */
size_t rx_bytes(long bits, int64_t n);
int64_t rx_offset(long bits, int64_t first);
/* the sample -t names; SC01 packs four to a byte, so there it rounds down to one */
int64_t rx_first_sample(const rx_opts_t *o);
/* n samples from sample `first` of the file into x; -1 when the file does not hold them */
int rx_read(FILE *fp, long bits, int64_t first, int64_t n, void *x);
/* the peak over the mean of its floor; 0 without a floor */
double rx_peak_ratio(const gss_acq_peak_t *p);

#endif /* CLI_RX_H */
