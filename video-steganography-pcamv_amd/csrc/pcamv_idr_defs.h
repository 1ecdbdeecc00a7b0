/*
 * pcamv_idr_defs.h -- what the IDR coder (pcamv_idr.h), its kernels (pcamv_idr.hip) and the library's host side (pcamv_gpu.hip) share:
 * the sizes, the slice header of an IDR I slice, the description of a picture and of a launch.  No HIP type; compiles for the device
 * and for the host.  Behind pcamv_stream_write.h (the bit writer of the slice headers).
 */
#ifndef PCAMV_IDR_DEFS_H
#define PCAMV_IDR_DEFS_H
#include "pcamv_stream_write.h"

#define IDR_LEVEL_MAX 2063
#define IDR_NBLK 27             /* 0 Intra16x16DCLevel, 1..16 luma AC of block b - 1, 17..24 chroma AC (Cb 0..3, Cr 0..3), 25 / 26 chroma DC */
/* the longest macroblock: mb_type ue(<= 24) 9, chroma mode ue(<= 3) 5, mb_qp_delta 1, a block of 16 (SWV_BLK_BITS = 464), 24 blocks of
 * 15 (436 each, derived next to SWV_BLK_BITS), two of 4 (118): 15 + 464 + 10464 + 236 = 11179 bits */
#define IDR_MB_BITS 11179
#define IDR_SLOT_DWORDS 352
static_assert(IDR_MB_BITS <= 32 * IDR_SLOT_DWORDS, "a macroblock's bit string fits its slot");
#define IDR_NZ_BYTES 24         /* total_coeff of a macroblock's AC blocks: luma by luma4x4BlkIdx, Cb 0..3, Cr 0..3 */
#define IDR_HDR_MAX_BITS 192    /* first_mb 1, slice_type ue(7) 7, pps_id 17, frame_num 16, idr_pic_id ue(65535) 33, POC <= 16 + 1 or 2, redundant 1,
                                 * the two marking flags, slice_qp_delta 13, the idc 3 -- or, of a filtered picture, idc 0 and two offsets of 0: 3 again, and
                                 * nothing under a PPS without deblocking control; the general bound ue(2) se se is 5 --: 112 at the most, so a filtered
                                 * picture's unit is as long as the unfiltered one's or shorter, and idr_bound stands */
#define IDR_HDR_BYTES 24
#define IDR_AUD_BYTES 6

/* ---------------------------------------------------------------- slice header (7.3.3) of an IDR I slice */
/* first_mb_in_slice 0, slice_type 7, pps_id, frame_num 0, idr_pic_id, the POC elements of the POC type (all zero), redundant_pic_cnt 0 if
 * present, no_output_of_prior_pics_flag 0, long_term_reference_flag 0, slice_qp_delta, then what says whether the picture is filtered.
 * deblock 0: disable_deblocking_filter_idc 1.  deblock 1 (the picture goes through k_idr_deblock, pcamv_idr_deblock.h): under a PPS with
 * deblocking control idc 0 and both offsets 0 -- ue(0) se(0) se(0), 3 bits where idc 1 has 3, so the header is as long -- and under a
 * PPS without it nothing: the filter is on by inference (7.4.3), and the header is 3 bits shorter than any that deblock 0 writes.
 * Refused before anything is written, in this order: PCAMV_EINVAL for parameter sets out of range, nal_ref_idc outside 1 .. 3 (an IDR
 * picture is a reference), idr_pic_id outside 0 .. 65535, a QP outside 0 .. 51, deblock not 0 or 1; PCAMV_EUNSUP for weighted_pred (as the
 * P header's writer), for entropy_cabac (the slice data is CAVLC) and, with deblock 0 only, for a PPS without deblocking control (the
 * picture is not filtered, and must say so). */
SP_HD int pcamv_idr_header_write2(const pcamv_stream_params_t &P, int nal_ref_idc, int idr_pic_id, int slice_qp, int deblock, uint8_t *bits_out, int *n_bits)
{
    *n_bits = 0;
    if (!sws_params_ok(P)) return PCAMV_EINVAL;
    if (nal_ref_idc < 1 || nal_ref_idc > 3 || idr_pic_id < 0 || idr_pic_id > 65535 || slice_qp < 0 || slice_qp > 51 || (deblock != 0 && deblock != 1)) return PCAMV_EINVAL;
    if (P.weighted_pred || P.entropy_cabac || (!deblock && !P.deblocking_filter_control_present)) return PCAMV_EUNSUP;
    SwsBits b = {bits_out, 0, 0, 0};
    sws_ue(b, 0);                                                               /* first_mb_in_slice */
    sws_ue(b, 7);                                                               /* slice_type: I, and every slice of the picture is */
    sws_ue(b, (uint32_t)P.pps_id);
    sws_u(b, P.log2_max_frame_num, 0);                                          /* frame_num */
    sws_ue(b, (uint32_t)idr_pic_id);
    if (P.poc_type == 0) {
        sws_u(b, P.log2_max_poc_lsb, 0);
        if (P.pic_order_present) sws_se(b, 0);
    } else if (P.poc_type == 1 && !P.delta_pic_order_always_zero) {
        sws_se(b, 0);
        if (P.pic_order_present) sws_se(b, 0);
    }
    if (P.redundant_pic_cnt_present) sws_ue(b, 0);
    sws_u(b, 1, 0);                                                             /* no_output_of_prior_pics_flag */
    sws_u(b, 1, 0);                                                             /* long_term_reference_flag */
    sws_se(b, slice_qp - P.pic_init_qp);
    if (!deblock) sws_ue(b, 1);                                                 /* disable_deblocking_filter_idc */
    else if (P.deblocking_filter_control_present) { sws_ue(b, 0); sws_se(b, 0); sws_se(b, 0); }      /* ... 0, slice_alpha_c0_offset_div2, slice_beta_offset_div2 */
    *n_bits = sws_end(b);
    return 0;
}
SP_HD int pcamv_idr_header_write(const pcamv_stream_params_t &P, int nal_ref_idc, int idr_pic_id, int slice_qp, uint8_t *bits_out, int *n_bits)
{
    return pcamv_idr_header_write2(P, nal_ref_idc, idr_pic_id, slice_qp, 0, bits_out, n_bits);
}

/* ---------------------------------------------------------------- the picture and a wave's working memory */
struct IdrPic {
    const uint8_t *src[3];              /* the source, tightly packed w x h, w/2 x h/2 twice */
    uint8_t *rec[3];                    /* the unfiltered reconstruction, the same layout (k_idr_deblock filters it in place, behind the coder) */
    int mb_w, mb_h, qp, qpc, dz;        /* qpc: the chroma QP; dz: the intra dead zone, of 64 */
    uint8_t *nz;                        /* [n_mb][IDR_NZ_BYTES] */
    uint32_t *slots;                    /* [n_mb][IDR_SLOT_DWORDS] a macroblock's bits, bit 31 of a dword first */
    int *bits;                          /* [n_mb] their number; negative: the coder failed on this macroblock (never) */
    int *clamped;                       /* [n_mb] levels the clamp changed (optional: the host check) */
};
/* the bytes of an RBSP whose stop bit is bit end_bit */
SP_HD long long idr_rbsp_bytes(long long end_bit) { return (end_bit + 8) >> 3; }
/* a capacity that always fits: the RBSP of the longest macroblocks, as a unit with every third byte an emulation prevention byte */
SP_HD long long idr_bound(long long n_mb, int as_nal)
{
    const long long rbsp = (IDR_HDR_MAX_BITS + n_mb * IDR_MB_BITS + 8) / 8 + 1;
    return as_nal ? 5 + rbsp + rbsp / 2 + 1 : rbsp;
}

/* The contexts of one call.  Context i's source and reconstruction planes, size and chroma QP offset are those of the frame descriptor
 * Fs[i]; its working memory is that of its place i - g0 in its group: nz, slots, bits, pre ((n_mb + 1) words), rbsp (rbsp_stride bytes, a
 * multiple of 256) are the group's, one entry per place.  qpc_of[12 + offset] is the chroma QP at this QP.  Unit i goes to
 * bytes[off[i] .. off[i] + cap[i]), its length to len[i], its code to status[i]; first (streams: k_idr_slot's code) may be NULL. */
struct FrameDev;
struct IdrJobs {
    const FrameDev *Fs; const uint8_t *tab;
    uint8_t *nz; uint32_t *slots; int *bits; long long *pre; uint8_t *rbsp; long long rbsp_stride; int *bad;
    uint8_t hdr[IDR_HDR_BYTES]; uint8_t qpc_of[25]; int hdr_bits, nal_byte, as_nal, aud, n_mb, qp, dz;
    int deblock;                        /* the pictures go through the loop filter before they become the references */
    uint8_t *bytes; long long bytes_size;
    long long *off, *cap, *len; int *first, *status;
};
#endif
