/*
 * gss_stage.h — what the post-render stages (noise, jammers, echoes, the band-limit filter) share
 * on the host and in their launches: the output formats' sizes, the split of a range of samples
 * into a head, whole groups and a tail, the grid under the workgroup cap, and the host
 * statements' quantise/pack epilogue.  DESIGN.md §11.4 states the shape; its device side is
 * csrc/hip/gss_stage_dev.h.  A group is the samples of one wide store (4, 8, 16 for SC16, SC08,
 * SC01: 16, 16, 4 bytes out, read by 16-byte loads); an item is what an edge takes at a time (a
 * sample, or the 4 samples of an SC01 byte).
 */
#ifndef GSS_STAGE_H
#define GSS_STAGE_H

#include <stddef.h>
#include <stdint.h>
#include "gpssim_amd.h"
#include "gss_impair.h"

#define GSS_STAGE_GRID_MAX 2048          /* workgroups of one launch, at most */

GSS_IMP_HD int gss_stage_ns(int fmt) { return fmt == GSS_FMT_SC16 ? 4 : fmt == GSS_FMT_SC08 ? 8 : 16; }
GSS_IMP_HD int gss_stage_item(int fmt) { return fmt == GSS_FMT_SC01 ? 4 : 1; }

/* the output bytes of n samples (SC01: n a multiple of 4) */
GSS_IMP_HD size_t gss_fmt_bytes(size_t n, int fmt)
{
    return fmt == GSS_FMT_SC16 ? n * 4 : fmt == GSS_FMT_SC08 ? n * 2 : n / 4;
}

/* the least head (a multiple of the item, below 16 and at most n) after which the input is
   16-byte aligned and the output aligned to its store (16, 16, 4 bytes), and the whole groups
   from there; none (addresses that never line up): head = n, every sample by the edges */
GSS_IMP_HD void gss_stage_split(uintptr_t in, uintptr_t out, uint64_t n, int fmt, uint64_t *head,
                                uint64_t *groups)
{
    const uint64_t item = (uint64_t)gss_stage_item(fmt);
    *head = n;
    *groups = 0;
    for (uint64_t h = 0; h < 16 && h <= n; h += item)
        if ((in + 4 * h) % 16 == 0 &&
            (out + gss_fmt_bytes((size_t)h, fmt)) % (fmt == GSS_FMT_SC01 ? 4 : 16) == 0) {
            *head = h;
            *groups = (n - h) / (uint64_t)gss_stage_ns(fmt);
            break;
        }
}

/* the edge items beside `groups` whole groups */
GSS_IMP_HD uint64_t gss_stage_items(uint64_t n, uint64_t groups, int fmt)
{
    return (n - groups * (uint64_t)gss_stage_ns(fmt)) / (uint64_t)gss_stage_item(fmt);
}

/* workgroups of `threads` for the larger of two work counts, 1..GSS_STAGE_GRID_MAX: the kernels
   stride over what is left */
GSS_IMP_HD unsigned gss_stage_grid(uint64_t work_a, uint64_t work_b, unsigned threads)
{
    const uint64_t a = (work_a + threads - 1) / threads, b = (work_b + threads - 1) / threads;
    const uint64_t g = a > b ? a : b;
    return g < 1 ? 1u : g > GSS_STAGE_GRID_MAX ? (unsigned)GSS_STAGE_GRID_MAX : (unsigned)g;
}

/* the host statements' epilogue: component i (2 j for I, 2 j + 1 for Q) of level v to its place
   in `out`; SC01 gathers 8 components in *byte, MSB first (gpssim.c:2268-2274) */
GSS_IMP_HD void gss_imp_put(void *out, int fmt, size_t i, int32_t v, uint8_t *byte)
{
    if (fmt == GSS_FMT_SC16) {
        ((int16_t *)out)[i] = (int16_t)gss_imp_sc16(v);
    } else if (fmt == GSS_FMT_SC08) {
        ((int8_t *)out)[i] = (int8_t)gss_imp_sc08(v);
    } else {
        const int bit = (int)(i & 7);
        *byte = (uint8_t)((bit ? *byte : 0) | ((v > 0 ? 1 : 0) << (7 - bit)));
        if (bit == 7)
            ((uint8_t *)out)[i >> 3] = *byte;
    }
}

#endif /* GSS_STAGE_H */
