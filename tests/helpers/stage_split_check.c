/*
 * stage_split_check.c — csrc/common/gss_stage.h on its own: the head/groups split that the
 * launches of the post-render stages share (it decides which addresses take 16-byte accesses),
 * gss_fmt_bytes, gss_stage_grid and the host epilogue gss_imp_put.  The split is checked by its
 * properties over every format, every 2-byte input offset within 32 bytes, every output offset
 * within 16 (even ones for SC16), out == in for SC16, and every n in 0..80; it takes addresses,
 * so no memory is touched.  Test infrastructure only.
 *
 * usage: stage_split_check
 */
#include <stdio.h>
#include <string.h>
#include "../../gps-sdr-sim_amd/csrc/common/gss_stage.h"

static int fails;

#define CHECK(c, ...)                                                                              \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            if (fails++ < 20) {                                                                    \
                printf("FAIL %s: ", #c);                                                           \
                printf(__VA_ARGS__);                                                               \
                printf("\n");                                                                      \
            }                                                                                      \
        }                                                                                          \
    } while (0)

/* sample h starts a group: its input at a 16-byte boundary, its output at a store's */
static int lines_up(uintptr_t in, uintptr_t out, int fmt, uint64_t h)
{
    const uintptr_t oa = fmt == GSS_FMT_SC01 ? 4 : 16;
    const uintptr_t ob = fmt == GSS_FMT_SC16 ? 4 * h : fmt == GSS_FMT_SC08 ? 2 * h : h / 4;
    return (in + 4 * h) % 16 == 0 && (out + ob) % oa == 0;
}

static void split_case(uintptr_t in, uintptr_t out, int fmt, uint64_t n)
{
    const uint64_t ns = fmt == GSS_FMT_SC16 ? 4 : fmt == GSS_FMT_SC08 ? 8 : 16;
    const uint64_t item = fmt == GSS_FMT_SC01 ? 4 : 1;
    uint64_t head = ~0ull, groups = ~0ull;
    gss_stage_split(in, out, n, fmt, &head, &groups);
#define AT "fmt %d in %#lx out %#lx n %lu: head %lu groups %lu", fmt, (unsigned long)in,           \
           (unsigned long)out, (unsigned long)n, (unsigned long)head, (unsigned long)groups
    CHECK(head % item == 0 && head <= n, AT);
    if (head > n)
        return;
    CHECK(groups <= (n - head) / ns, AT);
    if (groups > (n - head) / ns)
        return;
    const uint64_t tail = n - head - groups * ns;
    CHECK(tail % item == 0, AT);
    for (uint64_t g = 0; g < groups; g++)
        CHECK(lines_up(in, out, fmt, head + g * ns), AT);
    /* no earlier head would do; and where one within reach does, it is taken, with every whole
       group after it */
    int reach = 0;
    for (uint64_t h = 0; h < 16 && h <= n; h += item) {
        if (h < head)
            CHECK(!lines_up(in, out, fmt, h), AT);
        reach |= lines_up(in, out, fmt, h);
    }
    if (reach)
        CHECK(head < 16 && lines_up(in, out, fmt, head) && tail < ns, AT);
    else
        CHECK(head == n && groups == 0, AT);
    /* the kernels' walk (groups, then edge item e at e item, past the body once beyond the head)
       takes every sample once */
    unsigned char seen[96];
    memset(seen, 0, sizeof seen);
    for (uint64_t g = 0; g < groups; g++)
        for (uint64_t s = 0; s < ns; s++)
            seen[head + g * ns + s]++;
    const uint64_t items = gss_stage_items(n, groups, fmt);
    CHECK(items == (head + tail) / item, AT);
    for (uint64_t e = 0; e < items && e * item < sizeof seen; e++) {
        const uint64_t j = e * item < head ? e * item : e * item + groups * ns;
        for (uint64_t s = 0; s < item && j + s < sizeof seen; s++)
            seen[j + s]++;
    }
    int once = 1;
    for (uint64_t j = 0; j < sizeof seen; j++)
        once &= seen[j] == (j < n ? 1 : 0);
    CHECK(once, AT);
    /* in place, SC16: the echo launch's rule, in closed form */
    if (out == in && fmt == GSS_FMT_SC16) {
        const uint64_t h = ((16 - in % 16) % 16) / 4;
        if (in % 4 == 0 && h <= n)
            CHECK(head == h && groups == (n - h) / 4, AT);
        else
            CHECK(head == n && groups == 0, AT);
    }
#undef AT
}

int main(void)
{
    static const int fmts[3] = {GSS_FMT_SC16, GSS_FMT_SC08, GSS_FMT_SC01};
    const uintptr_t base_in = 0x7f0000100000ull, base_out = 0x7f0000900000ull;
    long cases = 0;
    for (int f = 0; f < 3; f++) {
        const int fmt = fmts[f];
        for (int i = 0; i < 16; i++)
            for (uint64_t n = 0; n <= 80; n += fmt == GSS_FMT_SC01 ? 4 : 1) {
                for (int k = 0; k < 16; k += fmt == GSS_FMT_SC16 ? 2 : 1, cases++)
                    split_case(base_in + 2 * i, base_out + k, fmt, n);
                if (fmt == GSS_FMT_SC16) {
                    split_case(base_in + 2 * i, base_in + 2 * i, fmt, n);
                    cases++;
                }
            }
    }
    /* sizes */
    for (size_t n = 0; n <= 80; n += 4) {
        CHECK(gss_fmt_bytes(n, GSS_FMT_SC16) == 4 * n && gss_fmt_bytes(n, GSS_FMT_SC08) == 2 * n &&
              gss_fmt_bytes(n, GSS_FMT_SC01) * 4 == n, "n %zu", n);
    }
    CHECK(gss_fmt_bytes(7, GSS_FMT_SC16) == 28 && gss_fmt_bytes(7, GSS_FMT_SC08) == 14, "n 7");
    /* the grid: enough workgroups for the larger count, 1 at least, the cap at most */
    CHECK(gss_stage_grid(0, 0, 256) == 1 && gss_stage_grid(1, 0, 256) == 1 &&
          gss_stage_grid(256, 257, 256) == 2 && gss_stage_grid(513, 3, 256) == 3 &&
          gss_stage_grid(2048ull * 256, 0, 256) == 2048 &&
          gss_stage_grid(0, 2048ull * 256 + 1, 256) == 2048 &&
          gss_stage_grid(~0ull / 2, 7, 256) == 2048, "gss_stage_grid");
    /* the epilogue: clamps, and component i at byte i / 8, bit 7 - i % 8 */
    static const int32_t ramp[] = {-40000, -32769, -32768, -32767, -2049, -2048, -2047, -17, -16,
                                   -15,    -2,     -1,     0,      1,     2,     15,    16,  17,
                                   2031,   2032,   2047,   2048,   32766, 32767, 32768, 40000};
    enum { NR = sizeof ramp / sizeof ramp[0] };              /* 26: three bytes and two bits over */
    int16_t o16[NR];
    int8_t o08[NR];
    uint8_t o01[NR / 8 + 1], byte = 0;
    memset(o01, 0xA5, sizeof o01);
    for (size_t i = 0; i < NR; i++) {
        gss_imp_put(o16, GSS_FMT_SC16, i, ramp[i], &byte);
        gss_imp_put(o08, GSS_FMT_SC08, i, ramp[i], &byte);
    }
    for (size_t i = 0; i < NR; i++)
        gss_imp_put(o01, GSS_FMT_SC01, i, ramp[i], &byte);
    for (size_t i = 0; i < NR; i++) {
        const int32_t v = ramp[i], w = v >> 4;
        CHECK(o16[i] == (v < -32768 ? -32768 : v > 32767 ? 32767 : v), "sc16 of %d: %d", v, o16[i]);
        CHECK(o08[i] == (w < -128 ? -128 : w > 127 ? 127 : w), "sc08 of %d: %d", v, o08[i]);
        if (i < NR / 8 * 8)
            CHECK(((o01[i / 8] >> (7 - i % 8)) & 1) == (v > 0), "sc01 of %d (component %zu)", v, i);
    }
    CHECK(o01[NR / 8] == 0xA5, "sc01 wrote a byte before its eighth component");
    if (fails) {
        printf("stage_split_check: %d failures\n", fails);
        return 1;
    }
    printf("stage_split_check ok (%ld splits)\n", cases);
    return 0;
}
