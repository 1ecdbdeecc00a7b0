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
/* the longest Intra4x4 macroblock (pcamv_idr_i4x4.h): mb_type ue(0) 1, sixteen times prev_intra4x4_pred_mode_flag 0 and rem_intra4x4_pred_mode
 * u(3) 64, chroma mode ue(<= 3) 5, coded_block_pattern me(v) of codeNum <= 47 11, mb_qp_delta 1, sixteen blocks of 16 (464 each), eight
 * of 15 (436), two of 4 (118): 82 + 7424 + 3488 + 236 = 11230 bits, 51 more than an Intra16x16 one and still within the slot */
#define IDR_MB_BITS_I4 11230
static_assert(IDR_MB_BITS_I4 == 1 + 64 + 5 + 11 + 1 + 16 * 464 + 8 * 436 + 2 * 118, "the terms of the longest Intra4x4 macroblock");
static_assert(IDR_MB_BITS_I4 >= IDR_MB_BITS && IDR_MB_BITS_I4 <= 32 * IDR_SLOT_DWORDS, "an Intra4x4 macroblock's bit string fits the same slot");
#define IDR_I4_BIAS 24          /* cost4 = IDR_I4_BIAS * lambda + the sixteen winning costs: the coder's own rule, not measured */
#define IDR_MODE_BYTES 16       /* Intra4x4PredMode of a macroblock's sixteen blocks by luma4x4BlkIdx; sixteen 2s (DC) for Intra16x16 (8.3.1.1) */
#define IDR_NZ_BYTES 24         /* total_coeff of a macroblock's AC blocks: luma by luma4x4BlkIdx, Cb 0..3, Cr 0..3 */
#define IDR_HDR_MAX_BITS 192    /* first_mb 1, slice_type ue(7) 7, pps_id 17, frame_num 16, idr_pic_id ue(65535) 33, POC <= 16 + 1 or 2, redundant 1,
                                 * the two marking flags, slice_qp_delta 13, the idc 3 -- or, of a filtered picture, idc 0 and two offsets of 0: 3 again, and
                                 * nothing under a PPS without deblocking control; the general bound ue(2) se se is 5 --: 112 at the most, so a filtered
                                 * picture's unit is as long as the unfiltered one's or shorter, and idr_bound stands.  A slice behind the
                                 * first (pcamv_idr_header_write3) has first_mb_in_slice ue(< 2^20): 41 bits where the first slice has 1 */
static_assert(112 + 40 <= IDR_HDR_MAX_BITS, "the header of a slice with first_mb_in_slice up to 2^20 - 1 is bounded as the first slice's is");
#define IDR_HDR_BYTES 24
#define IDR_FIRST_MB_MAX ((1 << 20) - 1)
#define IDR_AUD_BYTES 6

/* ---------------------------------------------------------------- slice header (7.3.3) of an IDR I slice */
/* first_mb_in_slice (0 but in the later slices of a picture of several: header_write3), slice_type 7, pps_id, frame_num 0, idr_pic_id,
 * the POC elements of the POC type (all zero), redundant_pic_cnt 0 if present, no_output_of_prior_pics_flag 0, long_term_reference_flag 0, slice_qp_delta, then what says whether the picture is filtered.
 * deblock 0: disable_deblocking_filter_idc 1.  deblock 1 (the picture goes through k_idr_deblock, pcamv_idr_deblock.h): under a PPS with
 * deblocking control idc 0 and both offsets 0 -- ue(0) se(0) se(0), 3 bits where idc 1 has 3, so the header is as long -- and under a
 * PPS without it nothing: the filter is on by inference (7.4.3), and the header is 3 bits shorter than any that deblock 0 writes.
 * Refused before anything is written, in this order: PCAMV_EINVAL for parameter sets out of range, nal_ref_idc outside 1 .. 3 (an IDR
 * picture is a reference), idr_pic_id outside 0 .. 65535, a QP outside 0 .. 51, deblock not 0 or 1; PCAMV_EUNSUP for weighted_pred (as the
 * P header's writer), for entropy_cabac (the slice data is CAVLC) and, with deblock 0 only, for a PPS without deblocking control (the
 * picture is not filtered, and must say so).
 * header_write3: the same header of the slice that begins at macroblock first_mb, 0 .. IDR_FIRST_MB_MAX (else PCAMV_EINVAL, with the other
 * values): every slice of a picture says the same but for that element, so the headers of a picture differ in length. */
SP_HD int pcamv_idr_header_write3(const pcamv_stream_params_t &P, int nal_ref_idc, int idr_pic_id, int slice_qp, int deblock, long long first_mb, uint8_t *bits_out, int *n_bits)
{
    *n_bits = 0;
    if (!sws_params_ok(P)) return PCAMV_EINVAL;
    if (nal_ref_idc < 1 || nal_ref_idc > 3 || idr_pic_id < 0 || idr_pic_id > 65535 || slice_qp < 0 || slice_qp > 51 || (deblock != 0 && deblock != 1) ||
        first_mb < 0 || first_mb > IDR_FIRST_MB_MAX) return PCAMV_EINVAL;
    if (P.weighted_pred || P.entropy_cabac || (!deblock && !P.deblocking_filter_control_present)) return PCAMV_EUNSUP;
    SwsBits b = {bits_out, 0, 0, 0};
    sws_ue(b, (uint32_t)first_mb);                                              /* first_mb_in_slice */
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
SP_HD int pcamv_idr_header_write2(const pcamv_stream_params_t &P, int nal_ref_idc, int idr_pic_id, int slice_qp, int deblock, uint8_t *bits_out, int *n_bits)
{
    return pcamv_idr_header_write3(P, nal_ref_idc, idr_pic_id, slice_qp, deblock, 0, bits_out, n_bits);
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
    int slice_rows = 0;                 /* macroblock rows per slice; 0 (and anything from mb_h up): the picture is one slice */
    int i4x4 = 0;                       /* idr_mb4 (pcamv_idr_i4x4.h): 0 Intra16x16 only, 1 Intra4x4 where it costs less, 2 Intra4x4 everywhere */
    int lambda = 0;                     /* pcamv_lambda_tab[qp]: the weight of a mode's bits in the Intra4x4 trial */
    uint8_t *modes = nullptr;           /* [n_mb][IDR_MODE_BYTES]; only with i4x4 != 0 */
};
/* the bytes of an RBSP whose stop bit is bit end_bit */
SP_HD long long idr_rbsp_bytes(long long end_bit) { return (end_bit + 8) >> 3; }
/* a capacity that always fits: the RBSP of the longest macroblocks, as a unit with every third byte an emulation prevention byte */
/* (idr_bound_bits, idr_slice_rbsp_at_bits, idr_bound_slices_bits: the same of macroblocks of at most mb_bits bits -- IDR_MB_BITS, or
 * IDR_MB_BITS_I4 in a call that may code Intra4x4 macroblocks) */
SP_HD long long idr_bound_bits(long long n_mb, int as_nal, int mb_bits)
{
    const long long rbsp = (IDR_HDR_MAX_BITS + n_mb * mb_bits + 8) / 8 + 1;
    return as_nal ? 5 + rbsp + rbsp / 2 + 1 : rbsp;
}
SP_HD long long idr_bound(long long n_mb, int as_nal) { return idr_bound_bits(n_mb, as_nal, IDR_MB_BITS); }
SP_HD int idr_mb_bits_of(int i4x4) { return i4x4 ? IDR_MB_BITS_I4 : IDR_MB_BITS; }

/* ---------------------------------------------------------------- several slices per picture: the layout, stated once
 * A slice is slice_rows whole macroblock rows (the last one what is left), so a macroblock's left neighbour is always in its slice and
 * its top and top-left neighbours are there together or not at all.  S = idr_n_slices; slice s begins at macroblock idr_slice_first_mb and
 * holds idr_slice_n_mb.  In a place's prefix array slice s owns the n_mb(s) + 1 entries from idr_slice_pre_at -- its macroblocks' first
 * bits behind its own header, then the bit of its stop bit -- so the array has n_mb + S entries; its RBSP begins at byte
 * idr_slice_rbsp_at of the place's RBSP area, a multiple of 4 that leaves every slice before it room for the longest header, the longest
 * macroblocks, the stop bit and the padding to a whole dword: the area of S slices ends at idr_slice_rbsp_at(n_mb, S).  A slice is then
 * idr_pack_dword's and idr_unit's arguments with these offsets. */
#define IDR_SLICE_PAD_BYTES 40
static_assert(8 * IDR_SLICE_PAD_BYTES >= IDR_HDR_MAX_BITS + 8 + 31 + 32, "a slice's room: header, stop bit, padding to a dword, and the dword its macroblocks' bound rounds down by");
SP_HD int idr_rows_per_slice(int mb_h, int slice_rows) { return slice_rows <= 0 || slice_rows >= mb_h ? mb_h : slice_rows; }
SP_HD int idr_n_slices(int mb_h, int slice_rows) { const int r = idr_rows_per_slice(mb_h, slice_rows); return (mb_h + r - 1) / r; }
SP_HD int idr_slice_of_row(int mb_h, int slice_rows, int my) { return my / idr_rows_per_slice(mb_h, slice_rows); }
SP_HD int idr_slice_row0(int mb_h, int slice_rows, int s) { return s * idr_rows_per_slice(mb_h, slice_rows); }
SP_HD int idr_slice_first_mb(int mb_w, int mb_h, int slice_rows, int s) { return idr_slice_row0(mb_h, slice_rows, s) * mb_w; }
SP_HD int idr_slice_n_mb(int mb_w, int mb_h, int slice_rows, int s)
{
    const int r = idr_rows_per_slice(mb_h, slice_rows), y0 = s * r, y1 = y0 + r < mb_h ? y0 + r : mb_h;
    return (y1 - y0) * mb_w;
}
SP_HD long long idr_slice_pre_at(long long first_mb, int s) { return first_mb + s; }
SP_HD long long idr_slice_rbsp_at_bits(long long first_mb, int s, int mb_bits) { return (long long)IDR_SLICE_PAD_BYTES * s + 4 * ((first_mb * mb_bits + 31) / 32); }
SP_HD long long idr_slice_rbsp_at(long long first_mb, int s) { return idr_slice_rbsp_at_bits(first_mb, s, IDR_MB_BITS); }
/* a capacity that always fits the S units of a picture behind each other: the sum of idr_bound over its slices */
SP_HD long long idr_bound_slices_bits(int mb_w, int mb_h, int slice_rows, int as_nal, int mb_bits)
{
    const int S = idr_n_slices(mb_h, slice_rows);
    long long sum = 0;
    for (int s = 0; s < S; s++) sum += idr_bound_bits(idr_slice_n_mb(mb_w, mb_h, slice_rows, s), as_nal, mb_bits);
    return sum;
}
SP_HD long long idr_bound_slices(int mb_w, int mb_h, int slice_rows, int as_nal) { return idr_bound_slices_bits(mb_w, mb_h, slice_rows, as_nal, IDR_MB_BITS); }
/* a slice's header as the device reads it: the table of a call has S of them */
struct IdrSliceHdr { uint8_t hdr[IDR_HDR_BYTES]; int bits, pad; };

/* The contexts of one call.  Context i's source and reconstruction planes, size and chroma QP offset are those of the frame descriptor
 * Fs[i]; its working memory is that of its place i - g0 in its group: nz, slots, bits, pre ((n_mb + 1) words), rbsp (rbsp_stride bytes, a
 * multiple of 256) are the group's, one entry per place.  qpc_of[12 + offset] is the chroma QP at this QP.  Unit i goes to
 * bytes[off[i] .. off[i] + cap[i]), its length to len[i], its code to status[i]; first (streams: k_idr_slot's code) may be NULL.
 * Several slices (slice_rows gives S > 1): pre has n_mb + S entries per place and the RBSP area room for S slices (the layout above);
 * shdr is the S headers; ulen / uoff ([S] per place, the group's) are the units' lengths (k_idr_unit_len) and their offsets behind off[i]
 * (k_idr_place); units, if not NULL, is the streams' contexts, whose unit counter k_idr_place moves on by the S - 1 that
 * k_stream_commit does not count. */
struct FrameDev;
struct IdrJobs {
    const FrameDev *Fs; const uint8_t *tab;
    uint8_t *nz; uint32_t *slots; int *bits; long long *pre; uint8_t *rbsp; long long rbsp_stride; int *bad;
    uint8_t hdr[IDR_HDR_BYTES]; uint8_t qpc_of[25]; int hdr_bits, nal_byte, as_nal, aud, n_mb, qp, dz;
    int deblock;                        /* the pictures go through the loop filter before they become the references */
    uint8_t *bytes; long long bytes_size;
    long long *off, *cap, *len; int *first, *status;
    int slice_rows, n_slices; const IdrSliceHdr *shdr; long long *ulen, *uoff; SwsCtx *units;
    int i4x4, lambda, mb_bits; uint8_t *modes;          /* IdrPic's i4x4 and lambda; the bound of a macroblock's bits the RBSP offsets are laid out by; [n_mb][IDR_MODE_BYTES] per place */
};
#endif
