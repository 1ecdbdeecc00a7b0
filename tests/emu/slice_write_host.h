/*
 * slice_write_host.h -- TEST-ONLY: the device slice writer's control code (csrc/pcamv_slice_write.h) run on the CPU with scalar
 * primitives: motion compensation and the transform are pcamv_prims_emu.h's over raster padded planes.  Every piece of the working
 * memory a wave keeps in LDS is a heap block of exactly its size here, and so is the output, so that a sanitizer build reports any
 * index the control code gets wrong.  Used by slice_write_driver.cpp and tests/fuzz/check_slice_write.cpp.
 */
#ifndef SLICE_WRITE_HOST_H
#define SLICE_WRITE_HOST_H
#define PCAMV_HOST_EMU 1
#include <stdlib.h>
#include <string.h>
#include "pcamv_common.h"
#include "pcamv_prims_emu.h"
#include "pcamv_logic.h"
#include "pcamv_host_tables.h"
#include "pcamv_slice_write.h"

/* the picture a slice is written from: source planes, the padded reference planes in raster rows (four luma planes of stride x lines
 * one after the other, the two chroma planes of cstride x clines), records; flip (optional): the flip map in carrier order */
struct SwHostFrame {
    const pcamv_params_t *p; int qp;
    const uint8_t *fenc[3]; uint8_t *luma4, *cu, *cv;
    const pcamv_mb_t *mbs; const int8_t *flip; int n_flip;
};

/* out: a block of exactly cap bytes */
static inline int sw_host_write(const SwHostFrame &in, const uint8_t *hdr_bits, int n_bits, int i_frame, int nal_byte, int as_nal,
                                uint8_t *out, long long cap, long long *len, uint32_t *hash)
{
    FrameDev F = {};
    pcamv_frame_set_params(&F, in.p);
    pcamv_frame_set_qp(&F, in.p, in.qp);
    if (!F.b_cabac) return PCAMV_EUNSUP;
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
    SwState W;
    memset(&W, 0, sizeof(W));
    SpState &S = W.S;
    int8_t *init_p = (int8_t *)malloc(2 * SW_NCTX);
    uint8_t *trans = (uint8_t *)malloc(256), *rlps = (uint8_t *)malloc(512);
    memcpy(init_p, pcamv_cabac_init_p, 2 * SW_NCTX); memcpy(trans, pcamv_cabac_transition, 256); memcpy(rlps, pcamv_cabac_range_lps, 512);
    const SpTables T = {init_p, trans, rlps};
    S.ctx = (uint8_t *)malloc(SW_NCTX);
    S.cmv = (uint32_t *)malloc(48 * 4); S.cmvd = (uint32_t *)malloc(48 * 4); S.cref = (int8_t *)malloc(48); S.cnz = (uint8_t *)malloc(48);
    S.row = (uint8_t *)calloc((size_t)SP_ROW_BYTES * F.mb_w, 1); S.tl = (uint32_t *)malloc(4);
    W.obuf = (uint32_t *)malloc(SW_OBUF);
    MBLocal *L = (MBLocal *)calloc(1, sizeof(MBLocal));
    const SwHeader H = {hdr_bits, n_bits, i_frame, nal_byte};
    const int rc = pcamv_slice_write(W, T, F, L, in.mbs, in.flip, car_base, in.n_flip, H, as_nal, out, cap, len, hash);
    free(S.ctx); free(S.cmv); free(S.cmvd); free(S.cref); free(S.cnz); free(S.row); free(S.tl); free(W.obuf); free(L);
    free(init_p); free(trans); free(rlps); free(car_base);
    return rc;
}
#endif
