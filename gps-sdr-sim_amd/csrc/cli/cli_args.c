/*
 * cli_args.c — option surface of the reference (getopt string "e:u:g:c:l:o:s:b:T:t:d:iv",
 * gpssim.c:1756-1852), same validation messages and the same last-option-wins behaviour.
 */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include "cli_args.h"

#define USER_MOTION_SIZE_DEFAULT 3000
#define STATIC_MAX_DURATION 86400

void gss_cli_usage(void)
{
    fprintf(stderr,
            "Usage: gps-sdr-sim [options]\n"
            "Options:\n"
            "  -e <gps_nav>     RINEX navigation file for GPS ephemerides (required)\n"
            "  -u <user_motion> User motion file (dynamic mode)\n"
            "  -g <nmea_gga>    NMEA GGA stream (dynamic mode)\n"
            "  -c <location>    ECEF X,Y,Z in meters (static mode) e.g. 3967283.154,1022538.181,4872414.484\n"
            "  -l <location>    Lat,Lon,Hgt (static mode) e.g. 35.681298,139.766247,10.0\n"
            "  -t <date,time>   Scenario start time YYYY/MM/DD,hh:mm:ss\n"
            "  -T <date,time>   Overwrite TOC and TOE to scenario start time\n"
            "  -d <duration>    Duration [sec] (dynamic mode max: %.0f, static mode max: %d)\n"
            "  -o <output>      I/Q sampling data file (default: gpssim.bin)\n"
            "  -s <frequency>   Sampling frequency [Hz] (default: 2600000)\n"
            "  -b <iq_bits>     I/Q data format [1/8/16] (default: 16)\n"
            "  -i               Disable ionospheric delay for spacecraft scenario\n"
            "  -v               Show details about simulated channels\n",
            ((double)USER_MOTION_SIZE_DEFAULT) / 10.0, STATIC_MAX_DURATION);
}

static void set_start(gss_cli_t *c, int y, int m, int d, int hh, int mm, double sec)
{
    c->opt.has_start = 1;
    c->opt.start[0] = y; c->opt.start[1] = m; c->opt.start[2] = d;
    c->opt.start[3] = hh; c->opt.start[4] = mm;
    c->opt.start_sec = sec;
}

/* a finite number with nothing after it */
static int parse_real(const char *s, double *v)
{
    char *end = NULL;
    if (!s || !*s)
        return 1;
    *v = strtod(s, &end);
    return *end != '\0' || !isfinite(*v);
}

/* One --jam value into c->jam[c->n_jam]:
     cw,<js_db>,<f_hz>[,pulse,<period_s>,<duty>]
     sweep,<js_db>,<f0_hz>,<f1_hz>,<sweep_s>[,pulse,<period_s>,<duty>]
   at the rate the run uses (a multiple of 10 Hz, gpssim.c:1877-1881), by gss_jam_make. */
static int jam_option(gss_cli_t *c, const char *val)
{
    char buf[256], *f[9];
    int nf = 0;
    if (strlen(val) >= sizeof buf)
        goto bad;
    strcpy(buf, val);
    for (char *p = buf;; p++) {
        if (nf == 9)
            goto bad;
        f[nf++] = p;
        p = strchr(p, ',');
        if (!p)
            break;
        *p = '\0';
    }
    const int sweep = strcmp(f[0], "sweep") == 0;
    const int base = sweep ? 5 : 3;
    if ((!sweep && strcmp(f[0], "cw") != 0) || (nf != base && nf != base + 3) ||
        (nf == base + 3 && strcmp(f[base], "pulse") != 0))
        goto bad;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   /* js f0 f1 sweep_s period_s duty */
    if (parse_real(f[1], &v[0]) || parse_real(f[2], &v[1]))
        goto bad;
    if (sweep && (parse_real(f[3], &v[2]) || parse_real(f[4], &v[3]) || !(v[3] > 0.0)))
        goto bad;
    if (nf == base + 3 &&
        (parse_real(f[base + 1], &v[4]) || parse_real(f[base + 2], &v[5]) || !(v[4] > 0.0)))
        goto bad;
    const double fs = floor(c->opt.samp_freq / 10.0) * 10.0;
    if (gss_jam_make(fs, v[0], v[1], v[2], v[3], v[4], v[5], &c->jam[c->n_jam]))
        goto bad;
    c->n_jam++;
    return 0;
bad:
    fprintf(stderr, "ERROR: Invalid jammer (cw,<js_db>,<f_hz> or sweep,<js_db>,<f0_hz>,<f1_hz>,"
                    "<sweep_s>, then optionally ,pulse,<period_s>,<duty>).\n");
    return 1;
}

/* One --multipath value into c->echo[c->n_echo]:
     <prn|all>,<delay_m>,<atten_db>[,<phase_deg>[,<doppler_hz>]]
   at the rate the run uses (a multiple of 10 Hz, gpssim.c:1877-1881), by gss_echo_make. */
static int echo_option(gss_cli_t *c, const char *val)
{
    char buf[256], *f[6];
    int nf = 0;
    if (strlen(val) >= sizeof buf)
        goto bad;
    strcpy(buf, val);
    for (char *p = buf;; p++) {
        if (nf == 6)
            goto bad;
        f[nf++] = p;
        p = strchr(p, ',');
        if (!p)
            break;
        *p = '\0';
    }
    if (nf < 3 || nf > 5)
        goto bad;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};             /* prn delay_m atten_db phase_deg doppler_hz */
    if (strcmp(f[0], "all") != 0 &&
        (parse_real(f[0], &v[0]) || v[0] < 1.0 || v[0] > 32.0 || v[0] != floor(v[0])))
        goto bad;
    for (int i = 1; i < nf; i++)
        if (parse_real(f[i], &v[i]))
            goto bad;
    const double fs = floor(c->opt.samp_freq / 10.0) * 10.0;
    if (gss_echo_make(fs, (int)v[0], v[1], v[2], v[3], v[4], &c->echo[c->n_echo]))
        goto bad;
    c->n_echo++;
    return 0;
bad:
    fprintf(stderr, "ERROR: Invalid multipath echo (<prn|all>,<delay_m>,<atten_db>[,<phase_deg>"
                    "[,<doppler_hz>]]: PRN 1..32, delay 0..299.8 km, at most 12 dB of gain).\n");
    return 1;
}

/* --bandwidth=<hz>[,<taps>] into c->fir: a low-pass of two-sided width <hz> with <taps> taps (63
   by default) at the rate the run uses (a multiple of 10 Hz, gpssim.c:1877-1881), by
   gss_fir_make. */
static int fir_option(gss_cli_t *c, const char *val)
{
    char buf[128];
    double bw = 0.0, taps = 63.0;
    if (strlen(val) >= sizeof buf)
        goto bad;
    strcpy(buf, val);
    char *comma = strchr(buf, ',');
    if (comma) {
        *comma = '\0';
        if (parse_real(comma + 1, &taps) || taps < 3.0 || taps > 63.0 || taps != floor(taps))
            goto bad;
    }
    if (parse_real(buf, &bw))
        goto bad;
    const double fs = floor(c->opt.samp_freq / 10.0) * 10.0;
    if (gss_fir_make(fs, bw, (int)taps, &c->fir))
        goto bad;
    c->has_fir = 1;
    return 0;
bad:
    fprintf(stderr, "ERROR: Invalid bandwidth (<hz>[,<taps>]: 0 < hz <= the sample rate, an odd "
                    "number of taps in 3..63).\n");
    return 1;
}

/* The noise options into c->impair.
     --cn0=<dB-Hz>        sigma = 250 sqrt(fs / (2 10^(cn0/10))) LSB per component: 250 is the carrier
                          table's amplitude, so this is the C/N0 of a satellite at gain 128 (path
                          loss 1 at antenna boresight); fs as the run uses it, a multiple of 10 Hz
                          (gpssim.c:1877-1881)
     --noise-sigma=<LSB>  sigma directly
     --noise-shift=<s>    0..8, or auto (default): the least s with (4 sigma + 2047 + J) / 2^s <=
                          R, R = 32767 for -b 16 and 2047 for -b 8 (what >> 4 takes to the 8-bit
                          range), J = sum of the jammers' amp 250 / 65536 (0 without --jam) plus
                          2047 alpha_q16 / 65536 per echo (--multipath); 0 for -b 1, which keeps
                          only the sign
     --seed=<u64>         default 0
   With --jam, --multipath or --bandwidth and neither --cn0 nor --noise-sigma: sigma 0
   (--noise-shift is then accepted, --seed is not).  --bandwidth leaves the automatic shift as it
   is: the filter reads the shifted SC16 samples, which that shift fits into 16 bits, and its
   DC gain is 1. */
static int noise_options(gss_cli_t *c, const char *o_cn0, const char *o_sigma, const char *o_shift,
                         const char *o_seed)
{
    if (o_cn0 && o_sigma) {
        fprintf(stderr, "ERROR: --cn0 and --noise-sigma are mutually exclusive.\n");
        return 1;
    }
    if (!o_cn0 && !o_sigma) {
        if (o_seed || (o_shift && c->n_jam == 0 && c->n_echo == 0 && !c->has_fir)) {
            fprintf(stderr, "ERROR: --noise-shift and --seed need --cn0 or --noise-sigma.\n");
            return 1;
        }
        if (c->n_jam == 0 && c->n_echo == 0 && !c->has_fir)
            return 0;
    }
    double v = 0.0, q8 = 0.0;
    if (!o_cn0 && !o_sigma) {
        /* jammers, echoes or the filter alone: no noise */
    } else if (o_cn0) {
        if (parse_real(o_cn0, &v) || v < -100.0 || v > 200.0) {
            fprintf(stderr, "ERROR: Invalid C/N0.\n");
            return 1;
        }
        const double fs = floor(c->opt.samp_freq / 10.0) * 10.0;
        q8 = floor(256.0 * 250.0 * sqrt(fs / (2.0 * pow(10.0, v / 10.0))) + 0.5);
    } else {
        if (parse_real(o_sigma, &v) || v < 0.0) {
            fprintf(stderr, "ERROR: Invalid noise sigma.\n");
            return 1;
        }
        q8 = floor(256.0 * v + 0.5);
    }
    if (!(q8 <= (double)0x00FFFFFF)) {
        fprintf(stderr, "ERROR: Noise sigma out of range (at most 65535 LSB).\n");
        return 1;
    }
    c->impair.sigma_q8 = (uint32_t)q8;
    if (o_shift && strcmp(o_shift, "auto") != 0) {
        if (parse_real(o_shift, &v) || v < 0.0 || v > 8.0 || v != floor(v)) {
            fprintf(stderr, "ERROR: Invalid noise shift (0..8 or auto).\n");
            return 1;
        }
        c->impair.shift = (int32_t)v;
    } else {
        double peak = 4.0 * (q8 / 256.0) + 2047.0;
        for (int i = 0; i < c->n_jam; i++)
            peak += (double)c->jam[i].amp * 250.0 / 65536.0;
        for (int i = 0; i < c->n_echo; i++)
            peak += 2047.0 * (double)c->echo[i].alpha_q16 / 65536.0;
        const double room = c->opt.data_format == GSS_FMT_SC16 ? 32767.0 : 2047.0;
        int s = 0;
        while (c->opt.data_format != GSS_FMT_SC01 && s < 8 && peak > room * (double)(1 << s))
            s++;
        c->impair.shift = s;
    }
    c->impair.seed = 0;
    if (o_seed) {
        char *end = NULL;
        errno = 0;
        const unsigned long long u = strtoull(o_seed, &end, 0);
        if (!*o_seed || *o_seed == '-' || *o_seed == '+' || *o_seed == ' ' || *end != '\0' ||
            errno) {
            fprintf(stderr, "ERROR: Invalid seed.\n");
            return 1;
        }
        c->impair.seed = (uint64_t)u;
    }
    c->has_impair = 1;
    return 0;
}

int gss_cli_parse(int argc, char **argv, gss_cli_t *c)
{
    memset(c, 0, sizeof *c);
    strcpy(c->out_file, "gpssim.bin");
    c->opt.samp_freq = 2.6e6;
    c->opt.data_format = GSS_FMT_SC16;
    c->opt.duration = -1.0;                   /* → USER_MOTION_SIZE/10 */
    c->opt.user_motion_size = USER_MOTION_SIZE_DEFAULT;
    const char *ums = getenv("GSS_USER_MOTION_SIZE");   /* the reference's -DUSER_MOTION_SIZE */
    if (ums && atoi(ums) > 0)
        c->opt.user_motion_size = atoi(ums);

    /* --carrier=float|int (an extension: the reference chooses at compile time, gpssim.h:4) is
       taken out before the reference's getopt loop sees the arguments */
    char *av[argc + 1];
    int ac = 0;
    /* additive noise (extensions, taken out the same way): --cn0=<dB-Hz> or --noise-sigma=<LSB>,
       --noise-shift=<0..8|auto>, --seed=<u64>; resolved once -s and -b are known */
    const char *o_cn0 = NULL, *o_sigma = NULL, *o_shift = NULL, *o_seed = NULL;
    /* jammers (--jam=..., repeatable): resolved with them, in the order given */
    const char *o_jam[GSS_MAXJAM];
    int n_ojam = 0;
    /* multipath echoes (--multipath=..., repeatable): the same */
    const char *o_echo[GSS_MAXECHO];
    int n_oecho = 0;
    /* the front-end filter (--bandwidth=..., once) */
    const char *o_fir = NULL;
    for (int i = 0; i < argc; i++) {
        if (i > 0 && strncmp(argv[i], "--bandwidth=", 12) == 0) {
            if (o_fir) {
                fprintf(stderr, "ERROR: --bandwidth given twice.\n");
                return 1;
            }
            o_fir = argv[i] + 12;
            continue;
        }
        if (i > 0 && strncmp(argv[i], "--multipath=", 12) == 0) {
            if (n_oecho == GSS_MAXECHO) {
                fprintf(stderr, "ERROR: At most %d multipath echoes.\n", GSS_MAXECHO);
                return 1;
            }
            o_echo[n_oecho++] = argv[i] + 12;
            continue;
        }
        if (i > 0 && strncmp(argv[i], "--jam=", 6) == 0) {
            if (n_ojam == GSS_MAXJAM) {
                fprintf(stderr, "ERROR: At most %d jammers.\n", GSS_MAXJAM);
                return 1;
            }
            o_jam[n_ojam++] = argv[i] + 6;
            continue;
        }
        if (i > 0 && strncmp(argv[i], "--cn0=", 6) == 0) {
            o_cn0 = argv[i] + 6;
            continue;
        }
        if (i > 0 && strncmp(argv[i], "--noise-sigma=", 14) == 0) {
            o_sigma = argv[i] + 14;
            continue;
        }
        if (i > 0 && strncmp(argv[i], "--noise-shift=", 14) == 0) {
            o_shift = argv[i] + 14;
            continue;
        }
        if (i > 0 && strncmp(argv[i], "--seed=", 7) == 0) {
            o_seed = argv[i] + 7;
            continue;
        }
        if (i > 0 && strncmp(argv[i], "--carrier=", 10) == 0) {
            if (strcmp(argv[i] + 10, "int") == 0)
                c->opt.carrier_int = 1;
            else if (strcmp(argv[i] + 10, "float") == 0)
                c->opt.carrier_int = 0;
            else {
                fprintf(stderr, "ERROR: Invalid carrier mode (float or int).\n");
                return 1;
            }
            continue;
        }
        av[ac++] = argv[i];
    }
    av[ac] = NULL;
    argc = ac;
    argv = av;

    if (argc < 3) {
        gss_cli_usage();
        return 1;
    }
    int r, has_d = 0;
    /* 0, not 1: glibc then re-initialises all of getopt's state.  With 1 it keeps its pointer
       into the previous call's argv, which a library caller (the Python binding) has freed, and
       reads it as more options. */
    optind = 0;
    while ((r = getopt(argc, argv, "e:u:g:c:l:o:s:b:T:t:d:iv")) != -1) {
        switch (r) {
        case 'e':
            snprintf(c->nav_file, sizeof c->nav_file, "%s", optarg);
            break;
        case 'u':
            snprintf(c->motion_file, sizeof c->motion_file, "%s", optarg);
            c->opt.nmea = 0;
            break;
        case 'g':
            snprintf(c->motion_file, sizeof c->motion_file, "%s", optarg);
            c->opt.nmea = 1;
            break;
        case 'c':
            c->opt.has_xyz = 1;
            c->opt.has_llh = 0;
            sscanf(optarg, "%lf,%lf,%lf", &c->opt.xyz[0], &c->opt.xyz[1], &c->opt.xyz[2]);
            break;
        case 'l':
            c->opt.has_llh = 1;
            c->opt.has_xyz = 0;
            sscanf(optarg, "%lf,%lf,%lf", &c->opt.llh[0], &c->opt.llh[1], &c->opt.llh[2]);
            break;
        case 'o':
            snprintf(c->out_file, sizeof c->out_file, "%s", optarg);
            break;
        case 's':
            c->opt.samp_freq = atof(optarg);
            if (c->opt.samp_freq < 1.0e6) {
                fprintf(stderr, "ERROR: Invalid sampling frequency.\n");
                return 1;
            }
            break;
        case 'b':
            c->opt.data_format = atoi(optarg);
            if (c->opt.data_format != 1 && c->opt.data_format != 8 && c->opt.data_format != 16) {
                fprintf(stderr, "ERROR: Invalid I/Q data format.\n");
                return 1;
            }
            break;
        case 'T':
            c->opt.time_overwrite = 1;
            if (strncmp(optarg, "now", 3) == 0) {
                time_t now;
                time(&now);
                struct tm *gmt = gmtime(&now);
                set_start(c, gmt->tm_year + 1900, gmt->tm_mon + 1, gmt->tm_mday, gmt->tm_hour,
                          gmt->tm_min, (double)gmt->tm_sec);
                break;
            }
            /* fall through: -T with a date parses like -t (gpssim.c:1804-1835) */
        case 't': {
            int y = 0, m = 0, d = 0, hh = 0, mm = 0;
            double sec = 0.0;
            sscanf(optarg, "%d/%d/%d,%d:%d:%lf", &y, &m, &d, &hh, &mm, &sec);
            if (y <= 1980 || m < 1 || m > 12 || d < 1 || d > 31 || hh < 0 || hh > 23 || mm < 0 ||
                mm > 59 || sec < 0.0 || sec >= 60.0) {
                fprintf(stderr, "ERROR: Invalid date and time.\n");
                return 1;
            }
            set_start(c, y, m, d, hh, mm, floor(sec));
            break;
        }
        case 'd':
            c->opt.duration = atof(optarg);
            has_d = 1;
            break;
        case 'i':
            c->opt.iono_disable = 1;
            break;
        case 'v':
            c->opt.verbose = 1;
            break;
        case ':':
        case '?':
            gss_cli_usage();
            return 1;
        default:
            break;
        }
    }
    c->opt.nav_file = c->nav_file;
    c->opt.motion_file = c->motion_file[0] ? c->motion_file : NULL;
    if (has_d && c->opt.duration < 0.0) {
        fprintf(stderr, "ERROR: Invalid duration.\n");
        return 1;
    }
    for (int i = 0; i < n_ojam; i++)
        if (jam_option(c, o_jam[i]))
            return 1;
    for (int i = 0; i < n_oecho; i++)
        if (echo_option(c, o_echo[i]))
            return 1;
    if (o_fir && fir_option(c, o_fir))
        return 1;
    return noise_options(c, o_cn0, o_sigma, o_shift, o_seed);
}
