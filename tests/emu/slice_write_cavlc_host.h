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

/* the picture a slice is written from: source planes, the padded reference planes in raster rows (four luma planes of stride x lines
 * one after the other, the two chroma planes of cstride x clines), records; flip (optional): the flip map in carrier order */
struct SwvHostFrame {
    const pcamv_params_t *p; int qp;
    const uint8_t *fenc[3]; uint8_t *luma4, *cu, *cv;
    const pcamv_mb_t *mbs; const int8_t *flip; int n_flip;
};
/* what a run tells beside the bytes: clipped level escapes written, the longest block string appended (bits), P_L0 16x16
 * macroblocks without residual whose MV is the skip prediction */
struct SwvHostStats { int n_clip, max_block_bits, n_fold; };

/* out: a block of exactly cap bytes */
static inline int swv_host_write(const SwvHostFrame &in, const uint8_t *hdr_bits, int n_bits, int nal_byte, int as_nal,
                                 uint8_t *out, long long cap, long long *len, SwvHostStats *stats)
{
    FrameDev F = {};
    pcamv_frame_set_params(&F, in.p);
    pcamv_frame_set_qp(&F, in.p, in.qp);
    if (F.b_cabac) return PCAMV_EUNSUP;
    for (int k = 0; k < 3; k++) F.fenc[k] = in.fenc[k];
    const size_t lsz = (size_t)F.stride * F.lines;
    for (int k = 0; k < 4; k++) F.luma[k] = in.luma4 + k * lsz + (size_t)F.stride * PCAMV_PAD + PCAMV_PAD;
    F.chroma[0] = in.cu + (size_t)F.cstride * PCAMV_CPAD + PCAMV_CPAD;
    F.chroma[1] = in.cv + (size_t)F.cstride * PCAMV_CPAD + PCAMV_CPAD;
    int *car_base = NULL;
    if (in.flip) {
        car_base = (int *)malloc(sizeof(int) * F.n_mb);
        int k = 0, slots[16];
        for (int xy = 0; xy < F.n_mb; xy++) { car_base[xy] = k; k += carrier_slots(in.mbs[xy].i_type, in.mbs[xy].i_partition, in.mbs[xy].i_sub_partition, in.mbs[xy].used, slots); }
    }
    SwvState W;
    memset((void *)&W, 0, sizeof(W));
    SvState &S = W.S;
    uint8_t *tab = (uint8_t *)malloc(SV_TAB_BYTES);
    if (sv_build_tables(tab)) { free(tab); free(car_base); return PCAMV_EINVAL; }
    S.vlc = (const uint16_t *)tab; S.cbp_of = tab + SV_T_CBP;
    S.cmv = (uint32_t *)malloc(48 * 4); S.cref = (int8_t *)malloc(48); S.cnz = (uint8_t *)malloc(48);
    S.row = (uint8_t *)calloc((size_t)SV_ROW_BYTES * F.mb_w, 1); S.tl = (uint32_t *)malloc(4);
    W.blk = (uint32_t *)calloc(SWV_NBLK * SWV_BLK_DWORDS, 4); W.blen = (uint32_t *)calloc(SWV_NBLK, 4);
    W.obuf = (uint32_t *)malloc(SW_OBUF);
    MBLocal *L = (MBLocal *)calloc(1, sizeof(MBLocal));
    const SwHeader H = {hdr_bits, n_bits, 0, nal_byte};
    const int rc = pcamv_slice_write_cavlc(W, F, L, in.mbs, in.flip, car_base, in.n_flip, H, as_nal, out, cap, len);
    if (stats) { stats->n_clip = W.n_clip; stats->max_block_bits = W.max_bits; stats->n_fold = W.n_fold; }
    free(S.cmv); free(S.cref); free(S.cnz); free(S.row); free(S.tl); free(W.blk); free(W.blen); free(W.obuf); free(L);
    free(tab); free(car_base);
    return rc;
}
#endif
