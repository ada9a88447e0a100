/*
 * gss_lin.h — the fast path's render arithmetic, restated once for the three places that must
 * agree on it bit for bit: the GPU kernel (gss_lin_kernel, csrc/hip/gss_synth.hip), the host
 * proof that certifies blocks for it (csrc/host/linearize.c) and the CPU checker of the tests
 * (tests/helpers/lin_check.c).  The rows a wave of the kernel starts a segment from (the lines
 * evaluated at the segment start: gss_lin_row_at, gss_lin_chan_of, below) are stated here too,
 * built by the kernel in its set-up and checked on the CPU by tests/helpers/lin_rows.c; so are
 * the chunk records a wave makes from its row, once for its four chunks (gss_lin_chunk_rec,
 * checked by tests/helpers/lin_chunk_rec.c).
 *
 * A block's channel is described by two 64-bit integer lines (gss_lin_t): the carrier
 * X(p) = x0 + p*xs mod 2^64 [2^-64 cycle] and the code Z(p) = z0 + p*zs [2^-50 chip, unwrapped]
 * (linearize.c proves how close they stay to the reference's double recurrences,
 * gpssim.c:2212-2250).  The kernel does not evaluate them at every sample.  Samples are grouped
 * in chunks of GSS_LIN_CHUNK (block-relative, aligned), a chunk in GSS_LIN_CH steps of 64 (lane l
 * of step s renders sample p = c + 64 s + l), and each lane keeps code and carrier in ONE 64-bit
 * register P (code in the low word, 8.24 fixed point with byte 3 = chip mod 256; carrier in the
 * high word, 2^-32 cycle) that advances by one 64-bit add per step:
 *   anchor   P(c, l) = B(c) + L(l)  mod 2^64, from the chunk's base and the lane's offset
 *              B = hi32(X(c) + A) : lo32((Z(c) + Ac) >> 26)
 *              L = hi32(l xs + 2^31) : lo32((l zs) >> 26)
 *   step     P += dX : dC,   dX = hi32(64 xs + 2^31) [2^-32 cycle],
 *                            dC = (64 zs + 2^25) >> 26 [2^-24 chip]
 *            A = 2^31 - (GSS_LIN_CH - 1) e / 2 and Ac = 2^25 - (GSS_LIN_CH - 1) ec / 2 centre
 *            the steps' errors e = dX 2^32 - 64 xs and ec = dC 2^26 - 64 zs.
 *   Z(c) is the code line reduced at its wave segment's start (GSS_LIN_SEG samples, aligned)
 *   to the chip there mod 1023 (1023 for chip 0: gss_lin_e0), plus the fraction.
 *   LUT cell = high word >> 23, where every carry out of the low word (at the anchor add and at
 *   each step, one per 256 chips) adds 2^-32 cycle to the carrier; chip = (unwrapped low word
 *   >> 24) mod 1023.
 * Each rounding is at most one unit (half a unit where rounded to nearest) and the carries only
 * add, so the carrier is within (GSS_LIN_CH/2 + 3) 2^31 + (2 + (GSS_LIN_CH - 1) dC / 2^32) 2^32
 * and the code within (GSS_LIN_CH/2 + 3) 2^25 of the lines (GSS_LIN_KDEV_*, 2^-64 cycle and 2^-50 chip); the
 * proof adds these to its own line-versus-reference bound.
 * The kernel reads each step's chip sign from a 32-chip window (gss_lin_kernel): every lane's
 * chip of one step must lie in it, which linearize.c checks as 63 zs + 3 chips <= 31
 * (GSS_LIN_WIN_OK).
 */
#ifndef GSS_LIN_H
#define GSS_LIN_H

#include <stdint.h>

#ifndef GSS_LIN_CH
#define GSS_LIN_CH     16                      /* 64-sample steps per chunk                   */
#endif
#define GSS_LIN_CHUNK  (64 * GSS_LIN_CH)       /* samples per chunk (block-relative, aligned) */
#define GSS_LIN_SEG    4096                    /* samples per wave segment: the code line is
                                                  taken mod 1023 chips at each segment start   */

#if defined(__HIPCC__)
#define GSS_LIN_FN static __host__ __device__ inline
#else
#define GSS_LIN_FN static inline
#endif

#define GSS_LIN_CSH    26                      /* code line (2^-50 chip) >> 26 = 8.24 chips   */

/* per-step increments and the carrier's anchor offset */
GSS_LIN_FN uint32_t gss_lin_dx(uint64_t xs) { return (uint32_t)((xs * 64u + (1ull << 31)) >> 32); }
GSS_LIN_FN uint32_t gss_lin_dz(uint64_t zs)
{
    return (uint32_t)((zs * 64u + (1ull << (GSS_LIN_CSH - 1))) >> GSS_LIN_CSH);
}
GSS_LIN_FN uint64_t gss_lin_xa(uint64_t xs)
{
    const int64_t e = (int64_t)(((uint64_t)gss_lin_dx(xs) << 32) - xs * 64u);
    return (1ull << 31) - (uint64_t)((e * (GSS_LIN_CH - 1)) / 2);
}
/* the code's anchor offset Ac (rounding and centring), added to Z(c) before >> 26 */
GSS_LIN_FN uint64_t gss_lin_za(uint64_t zs)
{
    const int64_t ec = (int64_t)(((uint64_t)gss_lin_dz(zs) << GSS_LIN_CSH) - zs * 64u);
    return (1ull << (GSS_LIN_CSH - 1)) - (uint64_t)((ec * (GSS_LIN_CH - 1)) / 2);
}

/* the chip the code line is reduced to at a segment start: the chip there mod 1023, taken as 1023
   for chip 0 so that the (possibly negative) anchor offset keeps the reduced line positive */
GSS_LIN_FN uint32_t gss_lin_e0(uint64_t chips)
{
    const uint32_t e = (uint32_t)(chips % 1023u);
    return e ? e : 1023u;
}

/* worst-case distance of the kernel's values from the lines, in line units (2^-64 cycle,
   2^-50 chip) */
/* carrier: roundings plus the carries of the code word, at most one at the anchor and one per
   2^32 of code advance over the chunk's steps (zs: the code line's step, 2^-50 chip per sample) */
#define GSS_LIN_KDEV_CARR(zs)                                                                      \
    ((((uint64_t)GSS_LIN_CH / 2 + 3) << 31) +                                                     \
     ((2 + (((uint64_t)gss_lin_dz(zs) * (GSS_LIN_CH - 1)) >> 32)) << 32))
#define GSS_LIN_KDEV_CODE (((uint64_t)GSS_LIN_CH / 2 + 3) << (GSS_LIN_CSH - 1))
/* the 32-chip step window holds every lane's chip (zs in 2^-50 chip per sample, < 1 chip) */
#define GSS_LIN_WIN_OK(zs) ((zs) * 63u + (3ull << 50) <= (31ull << 50))

/* The chunk window table (gss_tw16_kernel, gss_lin_kernel): row r (a C/A table row) and chunk
   start chip E hold the 16 steps' 32-chip windows of a chunk whose code base zb has
   zb >> 50 = E; step s's window starts at extended chip E + ((s w) >> 4) - GSS_LIN_CBW_PRE, w =
   gss_lin_wstep16(n_per_blk) the nominal chip advance per 64-sample step in 1/16 chip (1.023 MHz
   over the sample rate).  One table serves every channel of a launch: a channel's true advance
   differs from w by its code Doppler (parts in 10^6) and the rounding of w, which
   gss_lin_win16_ok checks against the window's slack, per channel and block. */
#define GSS_LIN_TWE     2560                   /* chunk start chips per table row            */
#define GSS_LIN_CBW_PRE 2                      /* a window starts this far below E + (s w>>4) */
GSS_LIN_FN uint32_t gss_lin_wstep16(int n_per_blk)
{
    return (uint32_t)((104755200ull + (uint64_t)n_per_blk / 2) / (uint64_t)n_per_blk);
}
/* every lane's chip of every step lies in the step's table window, and every chunk's E is inside
   the table, for a channel of code step zs (2^-50 chip per sample) whose code line is reduced to
   at most chip 1024 at each wave segment start (gss_lin_e0) */
GSS_LIN_FN int gss_lin_win16_ok(uint64_t zs, int n_per_blk)
{
    const int64_t U = (int64_t)1 << 50, z = (int64_t)zs;
    /* the kernel's code within KDEV of its anchored line, plus the anchor's centring offset and
       a margin (all below 2^-23 chip) */
    const int64_t kd = (int64_t)GSS_LIN_KDEV_CODE + ((int64_t)1 << 27);
    const uint32_t w = gss_lin_wstep16(n_per_blk);
    if (zs == 0 || zs >= (uint64_t)U)
        return 0;
    for (int s = 0; s < GSS_LIN_CH; s++) {
        const int64_t f = (int64_t)(((uint64_t)s * w) >> 4) - GSS_LIN_CBW_PRE;
        if (64 * s * z - kd < f * U)                          /* lane 0 at or above the start */
            return 0;
        if (U + (64 * s + 63) * z + kd > (f + 32) * U)        /* lane 63 below the end        */
            return 0;
    }
    /* the last chunk of a segment starts 3 chunks after a base at most 1024 chips */
    return 1025 * U + (int64_t)(GSS_LIN_SEG - GSS_LIN_CHUNK) * z + kd < (int64_t)GSS_LIN_TWE * U;
}

/* the lane offset L(l) of gss_lin.h: carrier word (high) and code word (low) */
GSS_LIN_FN uint64_t gss_lin_lane(uint64_t xs, uint64_t zs, uint32_t l)
{
    const uint32_t lx = (uint32_t)(((uint64_t)l * xs + (1ull << 31)) >> 32);
    const uint32_t lz = (uint32_t)(((uint64_t)l * zs) >> GSS_LIN_CSH);
    return ((uint64_t)lx << 32) | lz;
}

/* ---- the segment rows: what a wave of gss_lin_kernel starts its GSS_LIN_SEG samples from ------
   Per (channel, wave segment) the lines are evaluated once at the segment start n0 (a multiple of
   GSS_LIN_SEG), so that the chunk loop needs no 128-bit arithmetic and no schedule search; per
   channel the step constants.  gss_lin_kernel builds them in its set-up, one lane per row. */
typedef struct {
    uint64_t x;                  /* X(n0) + gss_lin_xa(xs): the first chunk's carrier anchor base */
    uint64_t z;                  /* ((E0 << 50) | fraction) + gss_lin_za(zs): the first chunk's
                                    code anchor base, E0 = gss_lin_e0(chip at the segment start) */
    int32_t g01;                 /* signed gain at the start (low 16) and after pos1 (high 16)   */
    int32_t pos1;                /* sample of the first gain change in the segment, or INT32_MAX */
    uint32_t npatch;             /* patched samples of the channel inside the segment            */
    uint32_t pad;
} gss_lin_row;
typedef struct {
    uint64_t xs, zs;             /* the lines' per-sample steps                                  */
    uint64_t d;                  /* the 64-sample step dX : dC of P (gss_lin_dx : gss_lin_dz)    */
    uint32_t dq;                 /* window offset advance per step, 1/16 chip, rounded down      */
    uint32_t tab;                /* the channel's C/A table row                                  */
} gss_lin_chan;

GSS_LIN_FN uint64_t gss_lin_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

/* the carrier anchor base of the segment that starts at n0 */
GSS_LIN_FN uint64_t gss_lin_row_x(uint64_t x0, uint64_t xs, uint64_t n0)
{
    return x0 + n0 * xs + gss_lin_xa(xs);
}
/* the code anchor base: Z(n0) = z0 + n0 zs in 128 bits (hi : lo), its chips reduced by
   gss_lin_e0, the fraction kept */
GSS_LIN_FN uint64_t gss_lin_row_z(uint64_t z0, uint64_t zs, uint64_t n0)
{
    const uint64_t lo = z0 + n0 * zs;
    const uint64_t hi = gss_lin_mulhi(n0, zs) + (lo < z0 ? 1u : 0u);
    const uint32_t e0 = gss_lin_e0((hi << 14) | (lo >> 50));
    return (((uint64_t)e0 << 50) | (lo & ((1ull << 50) - 1))) + gss_lin_za(zs);
}
/* the gain pair and pos1 from the schedule gpos[i] <= p < gpos[i+1] -> gval[i] (ngc entries,
   gpos[0] = 0, unused = INT32_MAX); writes g01 and pos1 of *r */
GSS_LIN_FN void gss_lin_row_gain(gss_lin_row *r, const int32_t *gpos, const int32_t *gval, int ngc,
                                 int32_t n0)
{
    /* gpos ascends, so the entries at or before n0 are a prefix (the last of them holds the gain
       at n0) and the first entry after n0 is the next change.  Every entry is read, with no
       early exit: the kernel's loads are then independent of each other (one round trip) */
    int32_t g0 = gval[0], gn = 0, pn = INT32_MAX;
    for (int i = 1; i < ngc; i++) {
        const int32_t p = gpos[i], v = gval[i];
        g0 = p <= n0 ? v : g0;
    }
    for (int i = ngc - 1; i >= 1; i--) {
        const int32_t p = gpos[i], v = gval[i];
        gn = p > n0 ? v : gn;
        pn = p > n0 ? p : pn;
    }
    const int more = pn < n0 + GSS_LIN_SEG;            /* (unused entries: INT32_MAX, never) */
    const int32_t g1 = more ? gn : g0;
    r->g01 = (int32_t)(((uint32_t)g0 & 0xFFFFu) | ((uint32_t)g1 << 16));
    r->pos1 = more ? pn : INT32_MAX;
}
/* the patched samples (ppos, np entries) inside the segment */
GSS_LIN_FN uint32_t gss_lin_row_npatch(const int32_t *ppos, int np, int32_t n0)
{
    uint32_t n = 0;
    for (int j = 0; j < np; j++)
        n += ppos[j] >= n0 && ppos[j] < n0 + GSS_LIN_SEG;
    return n;
}
GSS_LIN_FN gss_lin_row gss_lin_row_at(uint64_t x0, uint64_t xs, uint64_t z0, uint64_t zs,
                                      const int32_t *gpos, const int32_t *gval, int ngc,
                                      const int32_t *ppos, int np, int32_t n0)
{
    gss_lin_row r;
    r.x = gss_lin_row_x(x0, xs, (uint64_t)n0);
    r.z = gss_lin_row_z(z0, zs, (uint64_t)n0);
    gss_lin_row_gain(&r, gpos, gval, ngc, n0);
    r.npatch = gss_lin_row_npatch(ppos, np, n0);
    r.pad = 0;
    return r;
}
GSS_LIN_FN gss_lin_chan gss_lin_chan_of(uint64_t xs, uint64_t zs, uint32_t ca_tbl)
{
    gss_lin_chan c;
    c.xs = xs;
    c.zs = zs;
    c.d = ((uint64_t)gss_lin_dx(xs) << 32) | gss_lin_dz(zs);
    c.dq = (uint32_t)((zs * 64u) >> 46);
    c.tab = ca_tbl;
    return c;
}

/* ---- the chunk records: what a wave's render loop takes per (channel, chunk) ------------------
   A wave renders its segment in GSS_LIN_SEG / GSS_LIN_CHUNK chunks.  Everything a chunk needs
   from a channel follows from the channel's segment row, its constants and the chunk index c
   alone, so gss_lin_kernel makes all of a wave's records in one pass after its set-up (lane
   16 c + k: chunk c of channel k). */
#define GSS_LIN_REC_GAIN  1u                   /* flags: the gain changes inside the chunk      */
#define GSS_LIN_REC_PATCH 2u                   /* flags: the segment holds patched samples      */
typedef struct {
    uint64_t B;                  /* the chunk's anchor base: carrier word (high) : code word (low) */
    uint32_t wa, wn;             /* byte offsets of the window-table rows of this chunk and the
                                    next (C/A row, code base chip clamped to the table)          */
    uint32_t flags;              /* GSS_LIN_REC_*                                                */
    int32_t g;                   /* the signed gain at the chunk's first sample                  */
} gss_lin_chunk;

/* byte offset of the window-table row of C/A row tab for a chunk whose code base is zb (clamped
   to the table; gss_lin_win16_ok keeps a certified channel inside it) */
GSS_LIN_FN uint32_t gss_lin_wrow(uint32_t tab, uint64_t zb)
{
    const uint32_t e = (uint32_t)(zb >> 50);
    return (tab * GSS_LIN_TWE + (e < GSS_LIN_TWE - 1u ? e : GSS_LIN_TWE - 1u)) *
           (uint32_t)(GSS_LIN_CH * sizeof(uint32_t));
}
/* chunk c (0 .. GSS_LIN_SEG / GSS_LIN_CHUNK - 1) of the segment that starts at block sample n0:
   the bases are the row's advanced by c chunks (c < 4: shifts and adds, mod 2^64 like the lines) */
GSS_LIN_FN void gss_lin_chunk_rec(const gss_lin_row *row, const gss_lin_chan *chan, int32_t n0,
                                  int c, gss_lin_chunk *rec)
{
    const uint64_t xc = chan->xs * (uint64_t)GSS_LIN_CHUNK, zc = chan->zs * (uint64_t)GSS_LIN_CHUNK;
    const uint64_t xb = row->x + ((c & 1) ? xc : 0u) + ((c & 2) ? xc << 1 : 0u);
    const uint64_t zb = row->z + ((c & 1) ? zc : 0u) + ((c & 2) ? zc << 1 : 0u);
    const int32_t nb0 = n0 + c * GSS_LIN_CHUNK;
    const int after = row->pos1 <= nb0;                 /* the gain changed before the chunk */
    const int inside = !after && row->pos1 < nb0 + GSS_LIN_CHUNK;
    rec->B = (xb & ~0xFFFFFFFFull) | (uint32_t)(zb >> GSS_LIN_CSH);
    rec->wa = gss_lin_wrow(chan->tab, zb);
    rec->wn = gss_lin_wrow(chan->tab, zb + zc);
    rec->flags = (inside ? GSS_LIN_REC_GAIN : 0u) | (row->npatch != 0 ? GSS_LIN_REC_PATCH : 0u);
    rec->g = after ? row->g01 >> 16 : (int32_t)(int16_t)(row->g01 & 0xFFFF);
}

/* the kernel's LUT cell and chip at block sample p (128-bit code line; the proof's, on the host
   and in gss_linearize_device) */
typedef struct {
    int cell, chip;
} gss_lin_kc;

GSS_LIN_FN gss_lin_kc gss_lin_kernel_at(uint64_t x0, uint64_t xs, uint64_t z0, uint64_t zs,
                                         int64_t p)
{
    const int64_t c = p & ~(int64_t)(GSS_LIN_CHUNK - 1);
    const int64_t l = p & 63, s = (p - c) >> 6;
    const uint64_t lane = gss_lin_lane(xs, zs, (uint32_t)l);
    /* code: the low word, unwrapped (no carries in), from the line reduced at the segment start */
    const int64_t n0 = p & ~(int64_t)(GSS_LIN_SEG - 1);
    const unsigned __int128 zn = (unsigned __int128)z0 + (unsigned __int128)(uint64_t)n0 * zs;
    const int64_t chips = (int64_t)(zn >> 50), e0 = gss_lin_e0((uint64_t)chips);
    const __int128 z = (__int128)z0 + (__int128)c * (__int128)zs -
                      (__int128)(chips - e0) * ((__int128)1 << 50);
    const unsigned __int128 zk = (unsigned __int128)((z + (int64_t)gss_lin_za(zs)) >> GSS_LIN_CSH);
    const uint64_t za = (uint64_t)(uint32_t)zk + (uint32_t)lane;       /* anchor add, carry */
    const uint64_t zw = (uint64_t)(uint32_t)za + (uint64_t)s * gss_lin_dz(zs);   /* low word */
    const unsigned __int128 kz = zk + (uint32_t)lane + (unsigned __int128)(uint64_t)s *
                                 gss_lin_dz(zs);
    /* carrier: the high word plus the low word's carries */
    const uint32_t xb = (uint32_t)((x0 + (uint64_t)c * xs + gss_lin_xa(xs)) >> 32);
    const uint32_t xk = xb + (uint32_t)(lane >> 32) + (uint32_t)(za >> 32) +
                        (uint32_t)s * gss_lin_dx(xs) + (uint32_t)(zw >> 32);
    gss_lin_kc r;
    r.cell = (int)(xk >> 23);
    r.chip = (int)((uint64_t)(kz >> 24) % 1023u);
    return r;
}

#endif /* GSS_LIN_H */
