/*
 * pcamv_param_sets.h -- SPS / PPS as control code that compiles for the device and for the host: the parameter-set units of a byte
 * stream parsed, resolved into the stream's table, and the slice header read under that table.
 *
 * On the device it is the body of k_pset_unit, k_pset_parse, k_pset_resolve and k_slice_header_sets (pcamv_slice.hip.h).  On the host it
 * is what tests/fuzz/check_param_sets.cpp compiles with the scalar form of SP_LANES, to be compared stream by stream with
 * pcamv_gpu_stream_param_sets and header by header with pcamv_gpu_parse_slice_header_sets (pcamv_mvsyntax.h), whose semantics these are
 * on every input, valid or not (include/pcamv_gpu.h states them).  No HIP type.
 *
 * The units are found by the index scan of pcamv_stream_index.h with SiTable::sel = SI_SEL_PSET: "slice unit" there then reads "unit of
 * nal_unit_type 7 or 8" (si_selected), the rest of the three steps is the same, and so is their independence of the order of wavefronts.
 *
 * The syntax walk (ps_read_sps, ps_read_pps) is written once, over a bit reader: the host definition instantiates it with the reader of
 * pcamv_gpu_parse_slice_header, which goes bit by bit; the device with PsBits, the 32-bit window reader of the slice-header kernel.  The
 * writers (ps_write_sps, ps_write_pps) are the inverse, over the bit writer of pcamv_stream_write.h.
 *
 * Nothing outside the RBSP is read; results leave through ordinary stores.
 */
#ifndef PCAMV_PARAM_SETS_H
#define PCAMV_PARAM_SETS_H
#include <string.h>
#include "pcamv_stream_index.h"
#include "pcamv_stream_write.h"

#if defined(__HIPCC__)
#define PS_M __host__ __device__
#else
#define PS_M
#endif

/* the window reader of pcamv_stream_index.h under the interface the walk reads through */
struct PsBits {
    ShBits b;
    PS_M uint32_t u(int n) { return sh_u(b, n); }
    PS_M uint64_t ue() { return sh_ue(b); }
    PS_M long long se() { return sh_se(b); }
    PS_M int failed() const { return b.bad; }
    PS_M long long at() const { return b.pos; }
};
/* a parameter-set unit of a stream, parsed: its code, what it is (7 / 8), and the members of the one or the other */
struct PsRec { int32_t code, type; pcamv_sps_t sps; pcamv_pps_t pps; };

SP_HD int ps_high_profile(uint32_t p) { return p == 100 || p == 110 || p == 122 || p == 244 || p == 44 || p == 83 || p == 86 || p == 118 || p == 128; }
/* what a 32-bit element without a range is kept as */
SP_HD int32_t ps_i32(uint64_t v) { const uint32_t w = (uint32_t)v; int32_t r; memcpy(&r, &w, 4); return r; }

#define PS_READ(v, call) v = (call); if (B.failed()) return PCAMV_EINVAL
/* seq_parameter_set_data(), 7.3.2.1, up to vui_parameters_present_flag.  S is all zeros on entry; what it holds on failure is dropped */
template <class Bits> PS_M static inline int ps_read_sps(Bits &B, pcamv_sps_t &S)
{
    uint64_t e; long long s;
    PS_READ(e, B.u(8)); S.profile_idc = (int32_t)e;
    PS_READ(e, B.u(8)); S.constraint_flags = (int32_t)e;
    PS_READ(e, B.u(8)); S.level_idc = (int32_t)e;
    PS_READ(e, B.ue()); if (e > 31) return PCAMV_EINVAL;
    S.sps_id = (int32_t)e;
    S.chroma_format_idc = 1; S.bit_depth_luma = 8; S.bit_depth_chroma = 8;
    if (ps_high_profile((uint32_t)S.profile_idc)) {
        PS_READ(e, B.ue()); if (e != 1) return PCAMV_EUNSUP;                    /* chroma_format_idc */
        PS_READ(e, B.ue()); if (e != 0) return PCAMV_EUNSUP;                    /* bit_depth_luma_minus8 */
        PS_READ(e, B.ue()); if (e != 0) return PCAMV_EUNSUP;                    /* bit_depth_chroma_minus8 */
        PS_READ(e, B.u(1)); if (e) return PCAMV_EUNSUP;                         /* qpprime_y_zero_transform_bypass_flag */
        PS_READ(e, B.u(1)); if (e) return PCAMV_EUNSUP;                         /* seq_scaling_matrix_present_flag */
    }
    PS_READ(e, B.ue()); if (e > 12) return PCAMV_EINVAL;
    S.log2_max_frame_num = (int32_t)e + 4;
    PS_READ(e, B.ue()); if (e > 2) return PCAMV_EINVAL;
    S.poc_type = (int32_t)e;
    if (S.poc_type == 0) {
        PS_READ(e, B.ue()); if (e > 12) return PCAMV_EINVAL;
        S.log2_max_poc_lsb = (int32_t)e + 4;
    } else if (S.poc_type == 1) {
        PS_READ(e, B.u(1)); S.delta_pic_order_always_zero = (int32_t)e;
        PS_READ(s, B.se()); S.offset_for_non_ref_pic = (int32_t)s;
        PS_READ(s, B.se()); S.offset_for_top_to_bottom_field = (int32_t)s;
        PS_READ(e, B.ue()); if (e > 255) return PCAMV_EINVAL;
        S.num_ref_frames_in_poc_cycle = (int32_t)e;
        for (int k = 0; k < S.num_ref_frames_in_poc_cycle; k++) { PS_READ(s, B.se()); }         /* offset_for_ref_frame: not kept */
    }
    PS_READ(e, B.ue()); S.num_ref_frames = ps_i32(e);
    PS_READ(e, B.u(1)); S.gaps_in_frame_num_allowed = (int32_t)e;
    PS_READ(e, B.ue()); if (e + 1 > 65536) return PCAMV_EINVAL;
    S.mb_w = (int32_t)e + 1;
    PS_READ(e, B.ue()); if (e + 1 > 65536) return PCAMV_EINVAL;
    S.mb_h = (int32_t)e + 1;
    PS_READ(e, B.u(1)); if (!e) return PCAMV_EUNSUP;                            /* frame_mbs_only_flag (so no mb_adaptive_frame_field_flag) */
    S.frame_mbs_only = 1;
    PS_READ(e, B.u(1)); S.direct_8x8_inference = (int32_t)e;
    PS_READ(e, B.u(1)); S.frame_cropping = (int32_t)e;
    if (S.frame_cropping) {
        PS_READ(e, B.ue()); S.crop_left = ps_i32(e);
        PS_READ(e, B.ue()); S.crop_right = ps_i32(e);
        PS_READ(e, B.ue()); S.crop_top = ps_i32(e);
        PS_READ(e, B.ue()); S.crop_bottom = ps_i32(e);
    }
    PS_READ(e, B.u(1)); S.vui_parameters_present = (int32_t)e;
    return 0;
}
/* the position of the last 1 bit of rbsp[0, len), -1 if there is none: rbsp_stop_one_bit */
SP_HD long long ps_last_one(const uint8_t *rbsp, long long len)
{
    for (long long i = len - 1; i >= 0; i--)
        if (rbsp[i]) return 8 * i + 7 - __builtin_ctz((unsigned)rbsp[i]);
    return -1;
}
/* pic_parameter_set_rbsp(), 7.3.2.2; last_one as ps_last_one gives it */
template <class Bits> PS_M static inline int ps_read_pps(Bits &B, long long last_one, pcamv_pps_t &P)
{
    uint64_t e; long long s;
    PS_READ(e, B.ue()); if (e > 255) return PCAMV_EINVAL;
    P.pps_id = (int32_t)e;
    PS_READ(e, B.ue()); if (e > 31) return PCAMV_EINVAL;
    P.sps_id = (int32_t)e;
    PS_READ(e, B.u(1)); P.entropy_cabac = (int32_t)e;
    PS_READ(e, B.u(1)); P.pic_order_present = (int32_t)e;
    PS_READ(e, B.ue()); if (e > 7) return PCAMV_EINVAL;
    if (e) return PCAMV_EUNSUP;                                                 /* slice groups */
    P.num_slice_groups = 1;
    PS_READ(e, B.ue()); if (e > 31) return PCAMV_EINVAL;
    P.num_ref_idx_l0_default = (int32_t)e + 1;
    PS_READ(e, B.ue()); if (e > 31) return PCAMV_EINVAL;
    P.num_ref_idx_l1_default = (int32_t)e + 1;
    PS_READ(e, B.u(1)); P.weighted_pred = (int32_t)e;
    PS_READ(e, B.u(2)); P.weighted_bipred_idc = (int32_t)e;
    PS_READ(s, B.se()); if (s < -26 || s > 25) return PCAMV_EINVAL;
    P.pic_init_qp = 26 + (int32_t)s;
    PS_READ(s, B.se()); P.pic_init_qs = ps_i32((uint64_t)(s + 26));
    PS_READ(s, B.se()); if (s < -12 || s > 12) return PCAMV_EINVAL;
    P.chroma_qp_index_offset = (int32_t)s;
    PS_READ(e, B.u(1)); P.deblocking_filter_control_present = (int32_t)e;
    PS_READ(e, B.u(1)); P.constrained_intra_pred = (int32_t)e;
    PS_READ(e, B.u(1)); P.redundant_pic_cnt_present = (int32_t)e;
    P.second_chroma_qp_index_offset = P.chroma_qp_index_offset;
    if (last_one < B.at()) return PCAMV_EINVAL;                                 /* no rbsp_stop_one_bit at or behind the position */
    if (B.at() < last_one) {                                                    /* more_rbsp_data() */
        P.has_tail = 1;
        PS_READ(e, B.u(1)); if (e) return PCAMV_EUNSUP;                         /* transform_8x8_mode_flag */
        PS_READ(e, B.u(1)); if (e) return PCAMV_EUNSUP;                         /* pic_scaling_matrix_present_flag */
        PS_READ(s, B.se()); if (s < -12 || s > 12) return PCAMV_EINVAL;
        P.second_chroma_qp_index_offset = (int32_t)s;
    }
    return 0;
}
#undef PS_READ

/* one lane per unit: the RBSP of a unit of type 7 / 8 (code 0 so far) into its record */
SP_HD void ps_parse_unit(const uint8_t *rbsp, long long len, int nal_header, PsRec *R)
{
    PsRec r;
    memset(&r, 0, sizeof(r));
    r.type = nal_header & 31;
    PsBits B = {{rbsp, len, 8 * len, 0, 0}};
    if (len < 0 || len > PCAMV_PSET_UNIT_BYTES) r.code = PCAMV_EINVAL;
    else if (r.type == 7) r.code = ps_read_sps(B, r.sps);
    else r.code = ps_read_pps(B, ps_last_one(rbsp, len), r.pps);
    if (r.code) { const int code = r.code, type = r.type; memset(&r, 0, sizeof(r)); r.code = code; r.type = type; }
    *R = r;
}

SP_HD int ps_same(const int32_t *a, const int32_t *b, int words) { for (int k = 0; k < words; k++) if (a[k] != b[k]) return 0; return 1; }
SP_HD pcamv_stream_params_t ps_merge(const pcamv_sps_t &S, const pcamv_pps_t &P)
{
    pcamv_stream_params_t o;
    o.log2_max_frame_num = S.log2_max_frame_num; o.poc_type = S.poc_type; o.log2_max_poc_lsb = S.poc_type == 0 ? S.log2_max_poc_lsb : 4;
    o.delta_pic_order_always_zero = S.delta_pic_order_always_zero; o.pic_order_present = P.pic_order_present;
    o.redundant_pic_cnt_present = P.redundant_pic_cnt_present; o.num_ref_idx_l0_default = P.num_ref_idx_l0_default; o.weighted_pred = P.weighted_pred;
    o.entropy_cabac = P.entropy_cabac; o.pic_init_qp = P.pic_init_qp; o.deblocking_filter_control_present = P.deblocking_filter_control_present;
    o.pps_id = P.pps_id;
    return o;
}
/* one wavefront per stream: rules 1 and 3 to 5 of pcamv_param_sets_t over the stream's records rec[0, min(count, PCAMV_PSET_UNITS_MAX)),
 * count the stream's parameter-set units.  pre: a code the stream has already (the index refused it), 0 if none.  want_w / want_h: the
 * picture size the stream must have, 0: any.  The codes are looked at a lane each; the walk over at most 64 records is one lane's */
SP_HD void ps_resolve(const PsRec *rec, long long count, int pre, int want_w, int want_h, pcamv_param_sets_t *out)
{
    uint64_t failed = 0;
    const int n = count < 0 ? 0 : count > PCAMV_PSET_UNITS_MAX ? PCAMV_PSET_UNITS_MAX : (int)count;
    SP_LANES(l) { NU_VOTE(failed, l, l < n && rec[l].code != 0); }
    SP_LANES(l) if (l == 0) {
        pcamv_param_sets_t o;
        memset(&o, 0, sizeof(o));
        int rc = pre;
        if (!rc && count > PCAMV_PSET_UNITS_MAX) rc = PCAMV_EUNSUP;
        if (!rc && failed) rc = rec[__builtin_ctzll(failed)].code;
        int sps[PCAMV_PSET_SPS_MAX], pps[PCAMV_PSET_PPS_MAX], n_sps = 0, n_pps = 0;    /* the first unit of each id */
        for (int u = 0; u < n && !rc; u++) {
            const PsRec &r = rec[u];
            int found = -1;
            if (r.type == 7) {
                for (int k = 0; k < n_sps; k++) if (rec[sps[k]].sps.sps_id == r.sps.sps_id) found = sps[k];
                if (found >= 0) { if (!ps_same((const int32_t *)&rec[found].sps, (const int32_t *)&r.sps, (int)(sizeof(pcamv_sps_t) / 4))) rc = PCAMV_EUNSUP; }
                else if (n_sps == PCAMV_PSET_SPS_MAX) rc = PCAMV_EUNSUP;
                else sps[n_sps++] = u;
            } else {
                for (int k = 0; k < n_pps; k++) if (rec[pps[k]].pps.pps_id == r.pps.pps_id) found = pps[k];
                if (found >= 0) { if (!ps_same((const int32_t *)&rec[found].pps, (const int32_t *)&r.pps, (int)(sizeof(pcamv_pps_t) / 4))) rc = PCAMV_EUNSUP; }
                else if (n_pps == PCAMV_PSET_PPS_MAX) rc = PCAMV_EUNSUP;
                else pps[n_pps++] = u;
            }
        }
        if (!rc && !n_pps) rc = PCAMV_EINVAL;
        int of[PCAMV_PSET_PPS_MAX];                                             /* the SPS each PPS names */
        for (int k = 0; k < n_pps && !rc; k++) {
            of[k] = -1;
            for (int j = 0; j < n_sps; j++) if (rec[sps[j]].sps.sps_id == rec[pps[k]].pps.sps_id) of[k] = sps[j];
            if (of[k] < 0) rc = PCAMV_EINVAL;
        }
        for (int k = 1; k < n_pps && !rc; k++)
            if (rec[of[k]].sps.mb_w != rec[of[0]].sps.mb_w || rec[of[k]].sps.mb_h != rec[of[0]].sps.mb_h) rc = PCAMV_EUNSUP;
        if (!rc && (want_w || want_h) && (rec[of[0]].sps.mb_w != want_w || rec[of[0]].sps.mb_h != want_h)) rc = PCAMV_EUNSUP;
        if (!rc) {
            o.mb_w = rec[of[0]].sps.mb_w; o.mb_h = rec[of[0]].sps.mb_h; o.n_pps = n_pps;
            for (int k = 0; k < n_pps; k++) {                                   /* by pps_id ascending */
                int at = 0;
                for (int j = 0; j < n_pps; j++) if (rec[pps[j]].pps.pps_id < rec[pps[k]].pps.pps_id) at++;
                o.pps[at] = ps_merge(rec[of[k]].sps, rec[pps[k]].pps);
            }
        }
        o.status = rc;
        *out = o;
    }
}

/* pcamv_slice_header_read under a stream's sets.  *entropy: the entry's entropy mode, -1 where no entry was reached.  want_cabac >= 0: a
 * slice whose entry states the other mode is PCAMV_EUNSUP, judged where pps_id is */
SP_HD int pcamv_slice_header_read_sets(const uint8_t *rbsp, long long len, int nal_header, const pcamv_param_sets_t &T, int want_cabac, long long *start_bit,
                                       int *slice_qp, int *frame_num, int *entropy)
{
    *start_bit = -1; *slice_qp = -1; *frame_num = -1; *entropy = -1;
    if (T.status) return T.status;
    if (len < 0 || len > (1LL << 40)) return PCAMV_EINVAL;
    if (nal_header < 0 || (nal_header & 31) != 1) return PCAMV_EUNSUP;
    ShBits b = {rbsp, len, 8 * len, 0, 0};
    uint64_t e;
    e = sh_ue(b); if (b.bad) return PCAMV_EINVAL;
    if (e) return PCAMV_EUNSUP;                                                 /* first_mb_in_slice */
    e = sh_ue(b); if (b.bad) return PCAMV_EINVAL;
    if (e != 0 && e != 5) return PCAMV_EUNSUP;                                  /* slice_type */
    e = sh_ue(b); if (b.bad) return PCAMV_EINVAL;                               /* pps_id */
    int at = -1;
    for (int k = 0; k < T.n_pps && k < PCAMV_PSET_PPS_MAX; k++) if ((uint64_t)T.pps[k].pps_id == e) at = k;
    if (at < 0) return PCAMV_EUNSUP;
    *entropy = T.pps[at].entropy_cabac;
    if (want_cabac >= 0 && !T.pps[at].entropy_cabac != !want_cabac) return PCAMV_EUNSUP;
    return pcamv_slice_header_read(rbsp, len, nal_header, T.pps[at], start_bit, slice_qp, frame_num);
}

/* ---- the inverse: what the parsers read, written.  The codes are the parsers', member by member in syntax order */
SP_HD int ps_sps_ok(const pcamv_sps_t &S)
{
    if (S.profile_idc < 0 || S.profile_idc > 255 || S.constraint_flags < 0 || S.constraint_flags > 255 || S.level_idc < 0 || S.level_idc > 255) return PCAMV_EINVAL;
    if (S.sps_id < 0 || S.sps_id > 31) return PCAMV_EINVAL;
    if (S.chroma_format_idc != 1 || S.bit_depth_luma != 8 || S.bit_depth_chroma != 8 || S.transform_bypass || S.seq_scaling_matrix_present) return PCAMV_EUNSUP;
    if (S.log2_max_frame_num < 4 || S.log2_max_frame_num > 16 || S.poc_type < 0 || S.poc_type > 2) return PCAMV_EINVAL;
    if (S.poc_type == 0 && (S.log2_max_poc_lsb < 4 || S.log2_max_poc_lsb > 16)) return PCAMV_EINVAL;
    if (S.poc_type == 1 && (S.num_ref_frames_in_poc_cycle < 0 || S.num_ref_frames_in_poc_cycle > 255 || S.offset_for_non_ref_pic < -(1 << 30) ||
                            S.offset_for_non_ref_pic > (1 << 30) || S.offset_for_top_to_bottom_field < -(1 << 30) || S.offset_for_top_to_bottom_field > (1 << 30) ||
                            (S.delta_pic_order_always_zero != 0 && S.delta_pic_order_always_zero != 1))) return PCAMV_EINVAL;
    if (S.num_ref_frames < 0 || (S.gaps_in_frame_num_allowed != 0 && S.gaps_in_frame_num_allowed != 1)) return PCAMV_EINVAL;
    if (S.mb_w < 1 || S.mb_w > 65536 || S.mb_h < 1 || S.mb_h > 65536) return PCAMV_EINVAL;
    if (!S.frame_mbs_only) return PCAMV_EUNSUP;
    if ((S.direct_8x8_inference != 0 && S.direct_8x8_inference != 1) || (S.frame_cropping != 0 && S.frame_cropping != 1)) return PCAMV_EINVAL;
    if (S.frame_cropping && (S.crop_left < 0 || S.crop_right < 0 || S.crop_top < 0 || S.crop_bottom < 0)) return PCAMV_EINVAL;
    return 0;
}
/* rbsp: room for PCAMV_PSET_RBSP_MAX bytes; the RBSP's length in bytes, or a code */
SP_HD int ps_write_sps(const pcamv_sps_t &S, uint8_t *rbsp)
{
    const int rc = ps_sps_ok(S);
    if (rc) return rc;
    SwsBits b = {rbsp, 0, 0, 0};
    sws_u(b, 8, (uint32_t)S.profile_idc); sws_u(b, 8, (uint32_t)S.constraint_flags); sws_u(b, 8, (uint32_t)S.level_idc); sws_ue(b, (uint32_t)S.sps_id);
    if (ps_high_profile((uint32_t)S.profile_idc)) { sws_ue(b, 1); sws_ue(b, 0); sws_ue(b, 0); sws_u(b, 1, 0); sws_u(b, 1, 0); }
    sws_ue(b, (uint32_t)S.log2_max_frame_num - 4); sws_ue(b, (uint32_t)S.poc_type);
    if (S.poc_type == 0) sws_ue(b, (uint32_t)S.log2_max_poc_lsb - 4);
    else if (S.poc_type == 1) {
        sws_u(b, 1, (uint32_t)S.delta_pic_order_always_zero); sws_se(b, S.offset_for_non_ref_pic); sws_se(b, S.offset_for_top_to_bottom_field);
        sws_ue(b, (uint32_t)S.num_ref_frames_in_poc_cycle);
        for (int k = 0; k < S.num_ref_frames_in_poc_cycle; k++) sws_se(b, 0);
    }
    sws_ue(b, (uint32_t)S.num_ref_frames); sws_u(b, 1, (uint32_t)S.gaps_in_frame_num_allowed);
    sws_ue(b, (uint32_t)S.mb_w - 1); sws_ue(b, (uint32_t)S.mb_h - 1); sws_u(b, 1, 1); sws_u(b, 1, (uint32_t)S.direct_8x8_inference);
    sws_u(b, 1, (uint32_t)S.frame_cropping);
    if (S.frame_cropping) { sws_ue(b, (uint32_t)S.crop_left); sws_ue(b, (uint32_t)S.crop_right); sws_ue(b, (uint32_t)S.crop_top); sws_ue(b, (uint32_t)S.crop_bottom); }
    sws_u(b, 1, 0);                                                             /* vui_parameters_present_flag */
    sws_u(b, 1, 1);                                                             /* rbsp_trailing_bits */
    return (sws_end(b) + 7) / 8;
}
SP_HD int ps_pps_ok(const pcamv_pps_t &P)
{
    if (P.pps_id < 0 || P.pps_id > 255 || P.sps_id < 0 || P.sps_id > 31) return PCAMV_EINVAL;
    if ((P.entropy_cabac != 0 && P.entropy_cabac != 1) || (P.pic_order_present != 0 && P.pic_order_present != 1)) return PCAMV_EINVAL;
    if (P.num_slice_groups < 1 || P.num_slice_groups > 8) return PCAMV_EINVAL;
    if (P.num_slice_groups != 1) return PCAMV_EUNSUP;
    if (P.num_ref_idx_l0_default < 1 || P.num_ref_idx_l0_default > 32 || P.num_ref_idx_l1_default < 1 || P.num_ref_idx_l1_default > 32) return PCAMV_EINVAL;
    if ((P.weighted_pred != 0 && P.weighted_pred != 1) || P.weighted_bipred_idc < 0 || P.weighted_bipred_idc > 3) return PCAMV_EINVAL;
    if (P.pic_init_qp < 0 || P.pic_init_qp > 51 || P.pic_init_qs < 26 - (1 << 30) || P.pic_init_qs > 26 + (1 << 30) || P.chroma_qp_index_offset < -12 ||
        P.chroma_qp_index_offset > 12) return PCAMV_EINVAL;
    if ((P.deblocking_filter_control_present != 0 && P.deblocking_filter_control_present != 1) || (P.constrained_intra_pred != 0 && P.constrained_intra_pred != 1) ||
        (P.redundant_pic_cnt_present != 0 && P.redundant_pic_cnt_present != 1)) return PCAMV_EINVAL;
    if (P.transform_8x8_mode || P.pic_scaling_matrix_present) return PCAMV_EUNSUP;
    if (P.has_tail || P.second_chroma_qp_index_offset != P.chroma_qp_index_offset) return PCAMV_EINVAL;
    return 0;
}
SP_HD int ps_write_pps(const pcamv_pps_t &P, uint8_t *rbsp)
{
    const int rc = ps_pps_ok(P);
    if (rc) return rc;
    SwsBits b = {rbsp, 0, 0, 0};
    sws_ue(b, (uint32_t)P.pps_id); sws_ue(b, (uint32_t)P.sps_id); sws_u(b, 1, (uint32_t)P.entropy_cabac); sws_u(b, 1, (uint32_t)P.pic_order_present);
    sws_ue(b, 0); sws_ue(b, (uint32_t)P.num_ref_idx_l0_default - 1); sws_ue(b, (uint32_t)P.num_ref_idx_l1_default - 1);
    sws_u(b, 1, (uint32_t)P.weighted_pred); sws_u(b, 2, (uint32_t)P.weighted_bipred_idc);
    sws_se(b, P.pic_init_qp - 26); sws_se(b, (long long)P.pic_init_qs - 26); sws_se(b, P.chroma_qp_index_offset);
    sws_u(b, 1, (uint32_t)P.deblocking_filter_control_present); sws_u(b, 1, (uint32_t)P.constrained_intra_pred); sws_u(b, 1, (uint32_t)P.redundant_pic_cnt_present);
    sws_u(b, 1, 1);                                                             /* rbsp_trailing_bits */
    return (sws_end(b) + 7) / 8;
}
#endif
