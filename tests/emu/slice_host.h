/*
 * slice_host.h -- TEST-ONLY: what the four CPU runs of the device's slice control code (slice_parse_host.h, slice_parse_cavlc_host.h,
 * slice_write_host.h, slice_write_cavlc_host.h) share.  Every piece of the working memory a wave keeps in LDS is a heap block of
 * exactly its size -- never rounded up, pooled or sized for the other mode -- so that a sanitizer build reports any index the control
 * code gets wrong.
 */
#ifndef SLICE_HOST_H
#define SLICE_HOST_H
#include <stdlib.h>
#include <string.h>
#include "pcamv_slice_parse.h"

/* the neighbourhood of a slice's current macroblock (an SvState is an SpState): MVs, references and counts of the cache, the row
 * buffer of row_bytes (zeros), the MV above-left.  zeroed: the parsers start from zeros, the writers fill theirs before they read it */
static inline void slice_host_alloc(SpState &S, size_t row_bytes, int zeroed)
{
    S.cmv = (uint32_t *)malloc(48 * 4); S.cref = (int8_t *)malloc(48); S.cnz = (uint8_t *)malloc(48);
    S.row = (uint8_t *)calloc(row_bytes, 1); S.tl = (uint32_t *)malloc(4);
    if (zeroed) { memset(S.cmv, 0, 48 * 4); memset(S.cref, 0, 48); memset(S.cnz, 0, 48); S.tl[0] = 0; }
}
static inline void slice_host_free(SpState &S) { free(S.cmv); free(S.cref); free(S.cnz); free(S.row); free(S.tl); }

#ifdef SLICE_HOST_WRITER        /* defined by the writers' hosts, which run the scalar primitives and include pcamv_logic.h (FrameDev, carrier_slots) first */
/* the picture a slice is written from: source planes, the padded reference planes in raster rows (four luma planes of stride x lines
 * one after the other, the two chroma planes of cstride x clines), records; flip (optional): the flip map in carrier order */
struct SliceHostFrame {
    const pcamv_params_t *p; int qp;
    const uint8_t *fenc[3]; uint8_t *luma4, *cu, *cv;
    const pcamv_mb_t *mbs; const int8_t *flip; int n_flip;
};
static inline void slice_host_frame(FrameDev &F, const SliceHostFrame &in)
{
    pcamv_frame_set_params(&F, in.p);
    pcamv_frame_set_qp(&F, in.p, in.qp);
    for (int k = 0; k < 3; k++) F.fenc[k] = in.fenc[k];
    const size_t lsz = (size_t)F.stride * F.lines;
    for (int k = 0; k < 4; k++) F.luma[k] = in.luma4 + k * lsz + (size_t)F.stride * PCAMV_PAD + PCAMV_PAD;
    F.chroma[0] = in.cu + (size_t)F.cstride * PCAMV_CPAD + PCAMV_CPAD;
    F.chroma[1] = in.cv + (size_t)F.cstride * PCAMV_CPAD + PCAMV_CPAD;
}
/* the index of every macroblock's first carrier from the records (malloc; NULL without a flip map) */
static inline int *slice_host_car_base(const FrameDev &F, const SliceHostFrame &in)
{
    if (!in.flip) return NULL;
    int *car_base = (int *)malloc(sizeof(int) * F.n_mb);
    int k = 0, slots[16];
    for (int xy = 0; xy < F.n_mb; xy++) { car_base[xy] = k; k += carrier_slots(in.mbs[xy].i_type, in.mbs[xy].i_partition, in.mbs[xy].i_sub_partition, in.mbs[xy].used, slots); }
    return car_base;
}
#endif
#endif
