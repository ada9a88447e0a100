/* Test-only harness: the chunk records of csrc/common/gss_lin.h (gss_lin_chunk_rec: what a wave of
   gss_lin_kernel builds once for its four chunks, one lane per chunk and channel) exported for
   tests/test_lin_chunk_rec.py, which compares them with a restatement in Python integers, and
   gss_lin_win16_ok for the ends of the certified range of code steps. */
#include <stdint.h>
#include "../../gps-sdr-sim_amd/csrc/common/gss_lin.h"

/* row[5] = x, z, g01, pos1, npatch; chan[3] = xs, zs, tab; out[6] = B, wa, wn, flags, g, sizeof */
void lc_rec(const uint64_t *row, const uint64_t *chan, int32_t n0, int c, int64_t *out)
{
    gss_lin_row r;
    gss_lin_chan ch = gss_lin_chan_of(chan[0], chan[1], (uint32_t)chan[2]);
    gss_lin_chunk k;
    r.x = row[0];
    r.z = row[1];
    r.g01 = (int32_t)(uint32_t)row[2];
    r.pos1 = (int32_t)(uint32_t)row[3];
    r.npatch = (uint32_t)row[4];
    r.pad = 0;
    gss_lin_chunk_rec(&r, &ch, n0, c, &k);
    out[0] = (int64_t)k.B;
    out[1] = k.wa;
    out[2] = k.wn;
    out[3] = k.flags;
    out[4] = k.g;
    out[5] = (int64_t)sizeof k;
}

int lc_win16_ok(uint64_t zs, int n_per_blk) { return gss_lin_win16_ok(zs, n_per_blk); }
