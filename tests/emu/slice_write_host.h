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
#define SLICE_HOST_WRITER 1
#include "slice_host.h"

typedef SliceHostFrame SwHostFrame;

/* out: a block of exactly cap bytes */
static inline int sw_host_write(const SwHostFrame &in, const uint8_t *hdr_bits, int n_bits, int i_frame, int nal_byte, int as_nal,
                                uint8_t *out, long long cap, long long *len, uint32_t *hash)
{
    FrameDev F = {};
    slice_host_frame(F, in);
    if (!F.b_cabac) return PCAMV_EUNSUP;
    int *car_base = slice_host_car_base(F, in);
    SwState W;
    memset(&W, 0, sizeof(W));
    SpState &S = W.S;
    int8_t *init_p = (int8_t *)malloc(2 * SW_NCTX);
    uint8_t *trans = (uint8_t *)malloc(256), *rlps = (uint8_t *)malloc(512);
    memcpy(init_p, pcamv_cabac_init_p, 2 * SW_NCTX); memcpy(trans, pcamv_cabac_transition, 256); memcpy(rlps, pcamv_cabac_range_lps, 512);
    const SpTables T = {init_p, trans, rlps};
    S.ctx = (uint8_t *)malloc(SW_NCTX);
    S.cmvd = (uint32_t *)malloc(48 * 4);
    slice_host_alloc(S, (size_t)SP_ROW_BYTES * F.mb_w, 0);
    W.obuf = (uint32_t *)malloc(SW_OBUF);
    MBLocal *L = (MBLocal *)calloc(1, sizeof(MBLocal));
    const SwHeader H = {hdr_bits, n_bits, i_frame, nal_byte};
    const int rc = pcamv_slice_write(W, T, F, L, in.mbs, in.flip, car_base, in.n_flip, H, as_nal, out, cap, len, hash);
    slice_host_free(S);
    free(S.ctx); free(S.cmvd); free(W.obuf); free(L);
    free(init_p); free(trans); free(rlps); free(car_base);
    return rc;
}
#endif
