/*
 * slice_write_cavlc_host.h -- TEST-ONLY: the device CAVLC slice writer's control code (csrc/pcamv_slice_write_cavlc.h) run on the CPU
 * with scalar primitives: motion compensation and the transform are pcamv_prims_emu.h's over raster padded planes.  Every piece of
 * the working memory a wave keeps in LDS -- the per-lane block strings and their lengths included -- is a heap block of exactly its
 * size here, and so is the output, so that a sanitizer build reports any index the control code gets wrong.  Used by
 * slice_write_cavlc_driver.cpp and tests/fuzz/check_slice_write_cavlc.cpp.
 */
#ifndef SLICE_WRITE_CAVLC_HOST_H
#define SLICE_WRITE_CAVLC_HOST_H
#define PCAMV_HOST_EMU 1
#include <stdlib.h>
#include <string.h>
#include "pcamv_common.h"
#include "pcamv_prims_emu.h"
#include "pcamv_logic.h"
#include "pcamv_host_tables.h"
#include "pcamv_slice_write_cavlc.h"
#define SLICE_HOST_WRITER 1
#include "slice_host.h"

typedef SliceHostFrame SwvHostFrame;
/* what a run tells beside the bytes: clipped level escapes written, the longest block string appended (bits), P_L0 16x16
 * macroblocks without residual whose MV is the skip prediction */
struct SwvHostStats { int n_clip, max_block_bits, n_fold; };

/* out: a block of exactly cap bytes */
static inline int swv_host_write(const SwvHostFrame &in, const uint8_t *hdr_bits, int n_bits, int nal_byte, int as_nal,
                                 uint8_t *out, long long cap, long long *len, SwvHostStats *stats)
{
    FrameDev F = {};
    slice_host_frame(F, in);
    if (F.b_cabac) return PCAMV_EUNSUP;
    int *car_base = slice_host_car_base(F, in);
    SwvState W;
    memset((void *)&W, 0, sizeof(W));
    SvState &S = W.S;
    uint8_t *tab = (uint8_t *)malloc(SV_TAB_BYTES);
    if (sv_build_tables(tab)) { free(tab); free(car_base); return PCAMV_EINVAL; }
    S.vlc = (const uint16_t *)tab; S.cbp_of = tab + SV_T_CBP;
    slice_host_alloc(S, (size_t)SV_ROW_BYTES * F.mb_w, 0);
    W.blk = (uint32_t *)calloc(SWV_NBLK * SWV_BLK_DWORDS, 4); W.blen = (uint32_t *)calloc(SWV_NBLK, 4);
    W.obuf = (uint32_t *)malloc(SW_OBUF);
    MBLocal *L = (MBLocal *)calloc(1, sizeof(MBLocal));
    const SwHeader H = {hdr_bits, n_bits, 0, nal_byte};
    const int rc = pcamv_slice_write_cavlc(W, F, L, in.mbs, in.flip, car_base, in.n_flip, H, as_nal, out, cap, len);
    if (stats) { stats->n_clip = W.n_clip; stats->max_block_bits = W.max_bits; stats->n_fold = W.n_fold; }
    slice_host_free(S);
    free(W.blk); free(W.blen); free(W.obuf); free(L);
    free(tab); free(car_base);
    return rc;
}
#endif
