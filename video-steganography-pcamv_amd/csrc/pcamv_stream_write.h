/*
 * pcamv_stream_write.h -- the layer above a NAL unit on the SENDING side, as control code that compiles for the device and for the
 * host: the header of a P slice written, and the place of every picture's unit in a context's Annex B byte stream.
 *
 * On the device it is the body of k_stream_open, k_stream_slot, k_stream_commit and k_slice_headers_write (pcamv_slice.hip.h).  On the
 * host it is pcamv_gpu_write_slice_header, and what tests/fuzz/check_stream_write.cpp runs under the sanitizers against a case file.
 * No HIP type, no wave-wide operation: one lane does one context.
 *
 * pcamv_slice_header_write is the inverse of pcamv_slice_header_read (pcamv_stream_index.h): slice_header() (7.3.3) of a P slice,
 * element by element in the order x264_slice_header_write emits them (encoder/encoder.c:174-305), for frame macroblocks, one slice per
 * picture, no reordering, no memory management operations, cabac_init_idc 0 and one active reference.
 *
 * The most bits a header can take (PCAMV_SLICE_HDR_MAX_BITS, include/pcamv_gpu.h), element by element at the ends of the ranges that
 * are let through: first_mb_in_slice ue(0) 1; slice_type ue(5) 5; pps_id ue(255) 17; frame_num 16; the POC part is the longer of
 * poc_lsb 16 + se(+-2^30) 63 = 79 and two se(+-2^30) = 126 (|v| = 2^30 is ue(2^31 - 1) or ue(2^31): 31 zeros and 32 bits, the longest
 * code the readers take); redundant_pic_cnt ue(127) 15; the override flag and ue(0) 2; the reordering flag 1; the marking flag 1;
 * cabac_init_idc ue(0) 1; slice_qp_delta se(+-51) = ue(<= 102) 13; disable_deblocking_filter_idc ue(2) 3 and two se(+-6) = ue(<= 12)
 * of 7: 1 + 5 + 17 + 16 + 126 + 15 + 2 + 1 + 1 + 1 + 13 + 17 = 215 bits, 27 bytes; a context's slot of the header table is
 * PCAMV_SLICE_HDR_BYTES = 28, a multiple of 4.  (A header of the stream form has all POC deltas 0: 16 + 1 + 1 instead of 126.)
 *
 * A context's stream (SwsCtx) has three transitions:
 *   sws_open    its region of the caller's buffer is checked against the buffer, the caller's head (parameter sets and IDR picture,
 *               opaque) is copied to its start, the cursor stands behind it
 *   sws_slot    before the slice writer: the header of picture k into the writer's header table (the layout of WriteJobs::hdr,
 *               pcamv_slice_write_common.h), the access unit delimiter at the cursor, the place and capacity the writer gets
 *   sws_commit  behind the slice writer: the writer's length and status into the cursor, the caller's len[i], the picture counter
 *               and the status
 * Nothing outside [off, off + cap) of a context is written, and nothing at all for a context whose region sws_open refused.
 */
#ifndef PCAMV_STREAM_WRITE_H
#define PCAMV_STREAM_WRITE_H
#include "pcamv_stream_index.h"

#define SWS_HDR_WORDS 4         /* SW_HDR_WORDS of pcamv_slice_write_common.h: {byte offset of the bits, n_bits, i_frame, NAL header byte} */
#define SWS_AUD_BYTES 6
static_assert(PCAMV_SLICE_HDR_BYTES == ((PCAMV_SLICE_HDR_MAX_BITS + 7) / 8 + 3) / 4 * 4, "a slot holds the longest header and is whole dwords");

/* ---- bits, most significant first.  d == NULL: counted only */
struct SwsBits { uint8_t *d; int n; uint32_t acc; int fill; };          /* n: bits stored (whole bytes), fill < 8 more in acc */
SP_HD void sws_u(SwsBits &b, int n, uint32_t v)                         /* 0 <= n <= 32, v < 2^n */
{
    const uint64_t acc = (uint64_t)b.acc << n | v;
    int fill = b.fill + n;
    while (fill >= 8) {
        fill -= 8;
        if (b.d) b.d[b.n >> 3] = (uint8_t)(acc >> fill);
        b.n += 8;
    }
    b.acc = (uint32_t)(acc & (((uint64_t)1 << fill) - 1u)); b.fill = fill;
}
SP_HD void sws_ue(SwsBits &b, uint32_t v)                               /* v <= 2^31 */
{
    const int len = 32 - __builtin_clz(v + 1u);
    sws_u(b, len - 1, 0);
    sws_u(b, len, v + 1u);
}
SP_HD void sws_se(SwsBits &b, long long v) { sws_ue(b, (uint32_t)(v > 0 ? 2 * v - 1 : -2 * v)); }       /* |v| <= 2^30 */
SP_HD int sws_end(SwsBits &b)                                           /* the last byte zero-filled; the number of bits */
{
    const int n = b.n + b.fill;
    if (b.fill && b.d) b.d[b.n >> 3] = (uint8_t)(b.acc << (8 - b.fill));
    return n;
}

SP_HD int sws_params_ok(const pcamv_stream_params_t &P)                 /* the ranges pcamv_slice_header_read states */
{
    return P.log2_max_frame_num >= 4 && P.log2_max_frame_num <= 16 && P.poc_type >= 0 && P.poc_type <= 2 && P.log2_max_poc_lsb >= 4 && P.log2_max_poc_lsb <= 16 &&
           P.num_ref_idx_l0_default >= 1 && P.num_ref_idx_l0_default <= 32 && P.pic_init_qp >= 0 && P.pic_init_qp <= 51 && P.pps_id >= 0 && P.pps_id <= 255;
}
SP_HD int sws_delta_ok(long long v) { return v >= -(1LL << 30) && v <= (1LL << 30); }

/* The header of a P slice for the parameter sets P.  bits_out (NULL: nothing is stored, *n_bits alone) receives (*n_bits + 7) / 8 bytes,
 * the last one zero-filled, and not a byte more.  Every member of f is judged, whether P has its element written or not, and judged
 * before anything is written: PCAMV_EINVAL for a value out of range, then PCAMV_EUNSUP for weighted prediction (pred_weight_table);
 * *n_bits is 0 then */
SP_HD int pcamv_slice_header_write(const pcamv_stream_params_t &P, const pcamv_slice_fields_t &f, uint8_t *bits_out, int *n_bits)
{
    *n_bits = 0;
    if (!sws_params_ok(P)) return PCAMV_EINVAL;
    if (f.nal_ref_idc < 0 || f.nal_ref_idc > 3 || (f.slice_type != 0 && f.slice_type != 5) || f.frame_num < 0 || f.frame_num >= (1 << P.log2_max_frame_num) ||
        f.poc_lsb < 0 || f.poc_lsb >= (1 << P.log2_max_poc_lsb) || !sws_delta_ok(f.delta_pic_order_cnt_bottom) || !sws_delta_ok(f.delta_pic_order_cnt[0]) ||
        !sws_delta_ok(f.delta_pic_order_cnt[1]) || f.redundant_pic_cnt < 0 || f.redundant_pic_cnt > 127 || f.slice_qp < 0 || f.slice_qp > 51 ||
        f.disable_deblocking_filter_idc < 0 || f.disable_deblocking_filter_idc > 2 || f.slice_alpha_c0_offset_div2 < -6 || f.slice_alpha_c0_offset_div2 > 6 ||
        f.slice_beta_offset_div2 < -6 || f.slice_beta_offset_div2 > 6) return PCAMV_EINVAL;
    if (P.weighted_pred) return PCAMV_EUNSUP;
    SwsBits b = {bits_out, 0, 0, 0};
    sws_ue(b, 0);                                                               /* first_mb_in_slice */
    sws_ue(b, (uint32_t)f.slice_type);
    sws_ue(b, (uint32_t)P.pps_id);
    sws_u(b, P.log2_max_frame_num, (uint32_t)f.frame_num);
    if (P.poc_type == 0) {
        sws_u(b, P.log2_max_poc_lsb, (uint32_t)f.poc_lsb);
        if (P.pic_order_present) sws_se(b, f.delta_pic_order_cnt_bottom);
    } else if (P.poc_type == 1 && !P.delta_pic_order_always_zero) {
        sws_se(b, f.delta_pic_order_cnt[0]);
        if (P.pic_order_present) sws_se(b, f.delta_pic_order_cnt[1]);
    }
    if (P.redundant_pic_cnt_present) sws_ue(b, (uint32_t)f.redundant_pic_cnt);
    if (P.num_ref_idx_l0_default == 1) sws_u(b, 1, 0);                          /* num_ref_idx_active_override_flag */
    else { sws_u(b, 1, 1); sws_ue(b, 0); }                                      /* ... and num_ref_idx_l0_active_minus1: one reference */
    sws_u(b, 1, 0);                                                             /* ref_pic_list_reordering_flag_l0 */
    if (f.nal_ref_idc) sws_u(b, 1, 0);                                          /* adaptive_ref_pic_marking_mode_flag */
    if (P.entropy_cabac) sws_ue(b, 0);                                          /* cabac_init_idc */
    sws_se(b, f.slice_qp - P.pic_init_qp);
    if (P.deblocking_filter_control_present) {
        sws_ue(b, (uint32_t)f.disable_deblocking_filter_idc);
        if (f.disable_deblocking_filter_idc != 1) { sws_se(b, f.slice_alpha_c0_offset_div2); sws_se(b, f.slice_beta_offset_div2); }
    }
    *n_bits = sws_end(b);
    return 0;
}

/* ---- a context's stream */
struct SwsCtx { long long off, cap, cur, pic, units; int bad, pad; };   /* cur: bytes of the stream so far; pic: steps since the stream was opened;
                                                                         * units: slice units in it; bad: sws_open refused the region */
struct SwsSetup { pcamv_stream_params_t P; pcamv_stream_write_t W; };   /* what every context of a batch shares */
/* what sws_slot hands over: to the writer its place, to sws_commit the step's own code */
struct SwsSlot { long long off, cap; int first; };

/* what pcamv_gpu_batch_stream_open judges on the host before anything is queued */
SP_HD int sws_setup_ok(const SwsSetup &S)
{
    const pcamv_stream_write_t &W = S.W;
    if (!sws_params_ok(S.P) || W.nal_ref_idc < 1 || W.nal_ref_idc > 3 || (W.slice_type != 0 && W.slice_type != 5) || W.first_pic < 0 ||
        W.disable_deblocking_filter_idc < -1 || W.disable_deblocking_filter_idc > 2 || W.slice_alpha_c0_offset_div2 < -6 || W.slice_alpha_c0_offset_div2 > 6 ||
        W.slice_beta_offset_div2 < -6 || W.slice_beta_offset_div2 > 6 || (W.aud != 0 && W.aud != 1)) return PCAMV_EINVAL;
    return S.P.weighted_pred ? PCAMV_EUNSUP : 0;
}

/* the region [off, off + cap) of bytes[0, bytes_size) becomes context c's stream, head[0, head_len) its beginning; *len: its length */
SP_HD void sws_open(SwsCtx &c, uint8_t *bytes, long long bytes_size, long long off, long long cap, const uint8_t *head, long long head_len, long long *len)
{
    c.off = off; c.cap = cap; c.cur = 0; c.pic = 0; c.units = 0; c.pad = 0;
    c.bad = !(off >= 0 && cap >= 0 && cap <= bytes_size && off <= bytes_size - cap && head_len <= cap);
    if (!c.bad) {
        for (long long k = 0; k < head_len; k++) bytes[off + k] = head[k];
        c.cur = head_len;
    }
    *len = c.cur;
}

/* the members of picture k's header: counters as the reference's encoder advances them in a stream without B frames (encoder.c:1153-1158,
 * 2282, 2306); the deblocking idc the caller's, or with -1 the reference's rule (encoder.c:159-169) */
SP_HD pcamv_slice_fields_t sws_fields(const SwsSetup &S, long long k, int qp)
{
    const pcamv_stream_write_t &W = S.W;
    const long long pic = (long long)W.first_pic + k;
    pcamv_slice_fields_t f;
    f.nal_ref_idc = W.nal_ref_idc; f.slice_type = W.slice_type;
    f.frame_num = (int32_t)(pic & ((1LL << S.P.log2_max_frame_num) - 1)); f.poc_lsb = (int32_t)((2 * pic) & ((1LL << S.P.log2_max_poc_lsb) - 1));
    f.delta_pic_order_cnt_bottom = 0; f.delta_pic_order_cnt[0] = 0; f.delta_pic_order_cnt[1] = 0; f.redundant_pic_cnt = 0;
    f.slice_qp = qp;
    const int ab = W.slice_alpha_c0_offset_div2 < W.slice_beta_offset_div2 ? W.slice_alpha_c0_offset_div2 : W.slice_beta_offset_div2;
    f.disable_deblocking_filter_idc = W.disable_deblocking_filter_idc >= 0 ? W.disable_deblocking_filter_idc : 15 < qp + 2 * ab ? 0 : 1;
    f.slice_alpha_c0_offset_div2 = W.slice_alpha_c0_offset_div2; f.slice_beta_offset_div2 = W.slice_beta_offset_div2;
    return f;
}

/* Context i of n before the slice writer.  table: n entries of SWS_HDR_WORDS words, then n slots of PCAMV_SLICE_HDR_BYTES; entry i and
 * slot i are written.  The delimiter goes to the cursor if it and at least nothing else fit; a context without room for it, one whose
 * header cannot be made (a QP outside 0 .. 51) and one sws_open refused give the writer no room and their own code */
SP_HD SwsSlot sws_slot(const SwsSetup &S, const SwsCtx &c, uint8_t *bytes, int qp, int *table, int n, int i)
{
    const int at = n * SWS_HDR_WORDS * 4 + i * PCAMV_SLICE_HDR_BYTES;
    int n_bits = 0;
    const int rc = pcamv_slice_header_write(S.P, sws_fields(S, c.pic, qp), (uint8_t *)table + at, &n_bits);
    int *e = table + SWS_HDR_WORDS * i;
    e[0] = at; e[1] = n_bits; e[2] = (int)((uint32_t)S.W.first_i_frame + (uint32_t)c.pic); e[3] = S.W.nal_ref_idc << 5 | 1;
    SwsSlot s = {0, -1, PCAMV_EINVAL};                                  /* (a capacity below 0: the writer refuses the place and stores nothing) */
    if (c.bad) return s;
    const long long aud = S.W.aud ? SWS_AUD_BYTES : 0, room = c.cap - c.cur;
    s.off = c.off + c.cur; s.cap = 0; s.first = rc ? rc : PCAMV_ENOMEM;
    if (rc || room < aud) return s;
    if (aud) {
        uint8_t *d = bytes + s.off;
        d[0] = 0; d[1] = 0; d[2] = 0; d[3] = 1; d[4] = 0x09; d[5] = 0x30;   /* access_unit_delimiter_rbsp: primary_pic_type 1 (I, P), the stop bit */
    }
    s.off += aud; s.cap = room - aud; s.first = 0;
    return s;
}

/* Context c behind the slice writer, which wrote w_len bytes with code w_status at the place sws_slot gave it (first: that slot's code).
 * The picture counter moves on whatever happened; cursor and *len move only over a delimiter and a unit that are both there */
SP_HD void sws_commit(const SwsSetup &S, SwsCtx &c, int first, long long w_len, int w_status, long long *len, int *status)
{
    const int rc = c.bad ? PCAMV_EINVAL : first ? first : w_status;
    if (!rc) { c.cur += (S.W.aud ? SWS_AUD_BYTES : 0) + w_len; c.units++; }
    c.pic++;
    *len = c.cur; *status = rc;
}
#endif
