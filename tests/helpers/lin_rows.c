/* Test-only harness: the segment-row functions of csrc/common/gss_lin.h (what gss_lin_kernel
   builds per workgroup in its set-up) exported for tests/test_lin_rows.py, which compares them
   with a restatement in Python integers, and the kernel model gss_lin_kernel_at for the
   cross-check of the rows against it. */
#include <stdint.h>
#include "../../include/gpssim_amd.h"
#include "../../gps-sdr-sim_amd/csrc/common/gss_lin.h"

/* out[6] = x, z, g01, pos1, npatch, pad (the 32-bit fields zero- or sign-extended as declared) */
void lr_row(const gss_lin_t *l, int32_t n0, int64_t *out)
{
    const gss_lin_row r = gss_lin_row_at(l->x0, l->xs, l->z0, l->zs, l->gpos, l->gval, GSS_NGC,
                                         l->ppos, GSS_NPATCH, n0);
    out[0] = (int64_t)r.x;
    out[1] = (int64_t)r.z;
    out[2] = r.g01;
    out[3] = r.pos1;
    out[4] = r.npatch;
    out[5] = r.pad;
}

/* out[5] = xs, zs, d, dq, tab */
void lr_chan(const gss_lin_t *l, uint32_t ca_tbl, uint64_t *out)
{
    const gss_lin_chan c = gss_lin_chan_of(l->xs, l->zs, ca_tbl);
    out[0] = c.xs;
    out[1] = c.zs;
    out[2] = c.d;
    out[3] = c.dq;
    out[4] = c.tab;
}

uint64_t lr_lane(uint64_t xs, uint64_t zs, uint32_t l) { return gss_lin_lane(xs, zs, l); }

/* out[2] = cell, chip of the kernel model at block sample p */
void lr_kernel_at(const gss_lin_t *l, int64_t p, int32_t *out)
{
    const gss_lin_kc k = gss_lin_kernel_at(l->x0, l->xs, l->z0, l->zs, p);
    out[0] = k.cell;
    out[1] = k.chip;
}

int lr_sizes(int which) { return which ? (int)sizeof(gss_lin_chan) : (int)sizeof(gss_lin_row); }
