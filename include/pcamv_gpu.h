/*
 * pcamv_gpu.h -- C ABI of the MI355X P-frame analysis + MV-steganography library
 *                (libpcamv_gpu.so, built from video-steganography-pcamv_amd/csrc/).
 *
 * Frame-granular replacement for the per-macroblock work the reference does inside
 * x264_slice_write() (encoder/encoder.c:1176-2011) on the first of its two passes over a
 * P frame:
 *
 *   entry point                 replaces (reference file:line)
 *   --------------------------  -----------------------------------------------------------
 *   pcamv_gpu_open              vtable + table set-up in x264_encoder_open, encoder.c:694-766
 *                               (x264_cqm_init common/set.c:68, cost tables analyse.c:193-229)
 *   pcamv_gpu_set_ref           x264_fdec_filter_row's plane production, encoder.c:1038-1047:
 *                               x264_frame_expand_border (common/frame.c:246),
 *                               x264_frame_filter/hpel_filter (common/mc.c:453,167),
 *                               x264_frame_expand_border_filtered (common/frame.c:275)
 *   pcamv_gpu_upload_fenc       x264_frame_copy_picture (common/frame.c:183-220)
 *   pcamv_gpu_analyse_pframe    pass 1 of the raster MB loop, encoder.c:1240-1273:
 *                               x264_macroblock_cache_load (common/macroblock.c:914),
 *                               x264_macroblock_analyse (encoder/analyse.c:2555-3697) incl.
 *                               x264_me_search_ref (encoder/me.c:158), refine_subpel (me.c:715),
 *                               x264_ih_get_mv_cost (analyse.c:2391) and the pass-1 record
 *                               (analyse.c:3518-3689); the pass-1 x264_macroblock_encode
 *                               (encoder/macroblock.c:484) reconstruction
 *   pcamv_gpu_embed_pframe      cover/cost assembly + message + stc_embed + flip map,
 *                               encoder.c:1561-1855, embed.h:309-548
 *   pcamv_gpu_stc_extract       (no reference counterpart: extractor defined in SURVEY 8(c))
 *   pcamv_gpu_set_payload*      the message source, encoder.c:1838-1840 (rand() there: a caller's payload here)
 *   pcamv_gpu_*extract_*, rx_*  (no reference counterpart: the extractor is absent from the reference)
 *   pcamv_gpu_*_slices*,        (no reference counterpart) the receiver fed from stream bytes: CABAC and CAVLC P slices parsed on
 *   parse_pslice_*_device       the device, one wavefront per slice (k_parse_pslice, k_parse_pslice_cavlc), straight into the extractor
 *   pcamv_gpu_*_nals*,          the same fed NAL units: what a decoder's NAL layer undoes of x264_nal_encode (common/common.c:658-690), on
 *   nal_to_rbsp_device          the device, one wavefront per unit (k_nal_to_rbsp), in front of either parser
 *   pcamv_gpu_*_stream*,        the same fed a byte stream per context: Annex B start codes found (k_stream_scan, k_stream_place), the P slices'
 *   annexb_index, slice_header  headers read (k_slice_header: what x264_slice_header_write wrote, encoder.c:174-305), one slice unit per call
 *   pcamv_gpu_*write_*          the second pass' x264_macroblock_write_cabac + x264_cabac_encode_flush (encoder/cabac.c:781, common/cabac.c:908)
 *                               and x264_nal_encode (common/common.c:658): the P slice of a step written on the device (k_write_pslice);
 *                               the *_cavlc calls x264_macroblock_write_cavlc (encoder/cavlc.c:288) instead (k_write_pslice_cavlc)
 *   pcamv_gpu_close             x264_encoder_close's frees
 *
 * All functions return 0 on success and a negative PCAMV_E* code on error; the message is
 * available from pcamv_gpu_last_error().  One context per encoder, not re-entrant (the
 * reference's embedding path is single-threaded).  The caller owns every host
 * buffer it passes; the context owns all device memory.  There is NO CPU fallback: without a
 * HIP device every entry point fails with PCAMV_ENODEV.
 */
#ifndef PCAMV_GPU_H
#define PCAMV_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCAMV_EINVAL  (-1)
#define PCAMV_ENODEV  (-2)
#define PCAMV_ENOMEM  (-3)
#define PCAMV_EHIP    (-4)
#define PCAMV_EUNSUP  (-5)
#define PCAMV_EEOF    (-6)        /* a context's byte stream has no further slice unit (the receiver on byte streams) */

/* enum values are the reference's own (x264.h:106-111, common/macroblock.h mb_class_e / mb_partition_e) */
enum { PCAMV_ME_DIA = 0, PCAMV_ME_HEX = 1, PCAMV_ME_UMH = 2, PCAMV_ME_ESA = 3, PCAMV_ME_TESA = 4 };
enum { PCAMV_P_L0 = 4, PCAMV_P_8x8 = 5, PCAMV_P_SKIP = 6 };
enum { PCAMV_D_L0_4x4 = 0, PCAMV_D_L0_8x4 = 1, PCAMV_D_L0_4x8 = 2, PCAMV_D_L0_8x8 = 3,
       PCAMV_D_8x8 = 13, PCAMV_D_16x8 = 14, PCAMV_D_8x16 = 15, PCAMV_D_16x16 = 16 };
#define PCAMV_ANALYSE_I4x4      0x0001u   /* x264.h:97: intra 4x4 SATD analysis (only its cost is used, from subme 6 on) */
#define PCAMV_ANALYSE_PSUB16x16 0x0010u   /* x264.h:99  */
#define PCAMV_ANALYSE_PSUB8x8   0x0020u   /* x264.h:100 */

/* The subset of x264_param_t (x264.h:154-311) this path reads, with the reference's field
 * names and its post-x264_validate_parameters meaning (encoder.c:342-613). */
typedef struct pcamv_params_t {
    int32_t i_width, i_height;        /* luma size, multiples of 16                              */
    int32_t i_me_method;              /* analyse.i_me_method  (PCAMV_ME_*, all five)             */
    int32_t i_me_range;               /* analyse.i_me_range   (default 16, common.c:121); <= 16 with PCAMV_ME_TESA */
    int32_t i_subpel_refine;          /* analyse.i_subpel_refine, 1..7 (6 and 7 are the same for P frames: RD mode decision, incl.
                                         x264_rd_cost_part for sub-8x8 partitions); 8 / 9 (RD refinement of MVs: off in the fork's P frames) PCAMV_EUNSUP */
    int32_t i_mv_range;               /* analyse.i_mv_range after level lookup, encoder.c:558; >= 16 */
    int32_t b_chroma_me;              /* analyse.b_chroma_me  (default 1)                        */
    int32_t b_fast_pskip;             /* analyse.b_fast_pskip (default 1)                        */
    int32_t b_dct_decimate;           /* analyse.b_dct_decimate (default 1)                      */
    int32_t b_cabac;                  /* b_cabac (default 1): entropy coder whose sizes the RD mode decision uses */
    uint32_t inter;                   /* analyse.inter & (I4x4|PSUB16x16|PSUB8x8)                */
    int32_t i_chroma_qp_offset;       /* analyse.i_chroma_qp_offset                              */
    int32_t i_luma_deadzone[2];       /* analyse.i_luma_deadzone {inter,intra} = {21,11}         */
    int32_t i_tscale;                 /* temporal-candidate scale (common/macroblock.c:454); 256
                                         for consecutive P frames, 0 = previous frame was intra  */
    int32_t i_psy_rd;                 /* h->mb.i_psy_rd = FIX8(analyse.f_psy_rd) (encoder.c:515): 256 by default from subme 6 on,
                                         0 below; the caller also lowers i_chroma_qp_offset as encoder.c:520-521 does */
} pcamv_params_t;

/* One macroblock of the pass-1 record: the members of h->info.cache[] (common/common.h:585-603) that this path produces, under
 * their names and with their meaning; the ORDER of the members differs and the reference's (anonymous) struct carries more
 * (intra fields), so a host copies member by member (integration/pcamv_x264_glue.c).  mv[] / ref[] use x264's block-index
 * order 0 1 4 5 / 2 3 6 7 / 8 9 12 13 / 10 11 14 15 (analyse.c:2893-2898). */
typedef struct pcamv_mb_t {
    int32_t i_type;                   /* PCAMV_P_L0 | PCAMV_P_8x8 | PCAMV_P_SKIP                 */
    int32_t i_partition;              /* PCAMV_D_16x16 | 16x8 | 8x16 | 8x8                       */
    int32_t i_qp;
    uint8_t i_sub_partition[4];
    int8_t  ref[16];
    int16_t mv[16][2];
    int16_t mv_stego[16][2];
    int32_t inter_stego_cost[16];
    int16_t pskip_mv[2];              /* pskip_mv_ (encoder.c:1265)                              */
    int16_t mvr16[2];                 /* h->mb.mvr[0][0][mb]: the 16x16 search result            */
    uint8_t used;
    uint8_t pad[3];
} pcamv_mb_t;

/* Per-frame embedding vectors (h->info.cover/rho_final/message/stego/filp, common.h:604-617).
 * The caller allocates each array with room for 16 * mb_count entries. */
typedef struct pcamv_embed_t {
    int32_t  n;                       /* number of carrier MVs (h->info.length)                  */
    int32_t  m;                       /* number of message bits embedded                         */
    int32_t  stc_ok;                  /* stc_embed return value (ignored by the reference)       */
    int32_t  num_flip;
    uint8_t *cover;
    float   *rho;
    uint8_t *message;
    uint8_t *stego;
    int8_t  *flip;
} pcamv_embed_t;

typedef struct pcamv_ctx pcamv_ctx_t;
typedef struct pcamv_batch pcamv_batch_t;

int  pcamv_gpu_open(const pcamv_params_t *param, int device, pcamv_ctx_t **ctx);
void pcamv_gpu_close(pcamv_ctx_t *ctx);
const char *pcamv_gpu_last_error(const pcamv_ctx_t *ctx);

/* What a context remembers between calls (tests/test_gpu_call_order.py):
 *   - its QP is that of the last analysis or step (analyse_pframe, step_device, batch_step).  Pass 2, the loop filter and the slice
 *     writers work at it.  The probes (block_costs, rd_probe) take a QP of their own and leave the context as they found it: whatever
 *     runs after a probe computes what it would have computed without it;
 *   - pass2_pframe takes the context's state as it is now: the records in the record buffer, the source and the reference planes the
 *     context holds, the QP above.  It may take over the first pass' pixels of a macroblock whose motion did not change only while all
 *     of that is what the first pass saw.  A new source (upload_fenc, set_fenc_device), a host set_ref, new records (embed_records)
 *     and a step reported incomplete drop that reuse: every macroblock is then encoded again.  set_ref_device does not: its planes
 *     are produced by the next step, and a pass 2 before that step still runs against the reference before;
 *   - encode_idr and write_stream_idr leave a context as a host set_ref with no previous motion leaves it: the reconstruction of the IDR
 *     picture is the reference at once, its planes produced, the reuse of first-pass pixels dropped.  They take a QP of their own and
 *     leave the context's: pass2_pframe and the writers behind them behave as behind that set_ref.  With deblock 1 (encode_idr2,
 *     write_stream_idr2) that reference, and what fetch_recon / recon_device / get_ref_planes show, is the FILTERED picture; nothing of
 *     the choice outlives the call: the next IDR picture is filtered or not as its own call says. */

/* Source picture, I420, caller-owned host planes.  A pass 2 that follows encodes every macroblock on it. */
int pcamv_gpu_upload_fenc(pcamv_ctx_t *ctx, const uint8_t *const plane[3], const int stride[3]);

/* Reconstructed reference picture (already deblocked by the caller), I420 host planes, plus
 * the previous frame's final motion field for the temporal candidates
 * (x264_mb_predict_mv_ref16x16, common/macroblock.c:444-467): prev_mv is [mb_h*4][mb_w*4][2]
 * quarter-pel, prev_ref is [mb_h*2][mb_w*2]; both NULL when the reference is an I frame.
 * Produces the padded full/H/V/HV luma planes and padded chroma on the device, at once: a pass 2
 * that follows runs against the new reference and encodes every macroblock again. */
int pcamv_gpu_set_ref(pcamv_ctx_t *ctx, const uint8_t *const plane[3], const int stride[3],
                      const int16_t *prev_mv, const int8_t *prev_ref);

/* Read back the 4 padded luma planes produced by set_ref: out must hold 4*stride*lines
 * bytes; *stride = ALIGN(width+64,16), *lines = height+64, origin at (32,32).  The caller gets x264's
 * raster planes (filtered[0..3] with their borders); on the device they are kept in a strip layout
 * (DESIGN.md section 3), which this call undoes. */
int pcamv_gpu_get_ref_planes(pcamv_ctx_t *ctx, uint8_t *out, int *stride, int *lines);

/* Diagnostics: the same planes exactly as they lie in device memory -- the four luma planes in the strip layout, repeated
 * columns included (*luma_bytes = 4 * strips * 32 * lines), then the two padded chroma planes in raster rows (*chroma_bytes
 * = 2 * ALIGN(width/2+32,16) * (height/2+32)).  out may be NULL to ask for the sizes; else cap must be their sum. */
int pcamv_gpu_get_ref_strips(pcamv_ctx_t *ctx, uint8_t *out, size_t cap, size_t *luma_bytes, size_t *chroma_bytes);

/* Pass-1 analysis of the whole P frame at luma QP qp.  out_mb[mb_count] receives the record
 * (with embed != 0 also used / mv_stego / inter_stego_cost).  recon[3] (optional, tightly
 * packed w*h, w/2*h/2 x2) receives the pass-1 reconstruction before deblocking. */
int pcamv_gpu_analyse_pframe(pcamv_ctx_t *ctx, int qp, int embed, pcamv_mb_t *out_mb,
                             uint8_t *const recon[3]);

/* Embedding stage on the records of the last analyse call.  emrate as x264's --emrate
 * (encoder.c:1828-1836): 0 < r <= 1 bits per MV, r > 1 bits per frame.  message == NULL
 * draws the bits from the context's glibc-compatible rand() stream (seed 1 at open, as the
 * reference never calls srand, encoder.c:1838-1840) -- or, with a payload attached (pcamv_gpu_set_payload below), the
 * payload's next m bits; otherwise message[0..m) is used. */
int pcamv_gpu_embed_pframe(pcamv_ctx_t *ctx, float emrate, const uint8_t *message, int message_len,
                           pcamv_embed_t *out);

/* Apply the flip map to the record (pass-2 substitution, analyse.c:3001-3107): final MVs. */
int pcamv_gpu_final_mvs(pcamv_ctx_t *ctx, pcamv_mb_t *out_mb);

/* Pass 2 of the frame last analysed (analyse.c:2870-3107 + x264_macroblock_encode, then the loop filter
 * x264_frame_deblock_row, common/frame.c:627-798): final MVs = the record with mv_stego where flips[k] == 1
 * (k = carrier index in embedding order; flips == NULL: the flip map the last embed_pframe left on the
 * device), P_SKIP macroblocks take the skip prediction from their final neighbours; out_final (optional)
 * receives the record with the final MVs, recon[3] the reconstruction before the loop filter, deblocked[3]
 * after it.  The deblocked picture stays in the context's reconstruction planes (the next reference) and the
 * final motion field is what PCAMV_PREV_FIELD_INTERNAL hands to the next frame.  One QP per frame (CQP): that of
 * the last analysis or step, whatever QP a probe was given since.  The call takes the context's state as given --
 * the records in the record buffer (an analysis', or embed_records'), the source and the reference planes the
 * context holds now.  A macroblock whose motion did not change keeps the first pass' pixels only while all of that
 * is what the first pass saw and no second pass has run over them; otherwise it is encoded again.  A context that
 * has run no analysis or step has no QP, and nothing for this call to work on. */
int pcamv_gpu_pass2_pframe(pcamv_ctx_t *ctx, const uint8_t *flips, int n_flips, pcamv_mb_t *out_final,
                           uint8_t *const recon[3], uint8_t *const deblocked[3]);

/* Syndrome-trellis extraction (host side of the BER check): stego bits -> message bits (stc_extract, embed.h:340-393).
 * Sub-matrix widths 2..20 come from the code's tables; outside that range (payloads below 1/20 bit per MV, or 1 bit per MV) the
 * reference draws the columns from a process-wide LCG (embed.h:134-139) that every such frame advances, so the extractor needs
 * the generator's state: *lcg = state before this frame's embedding (1 for the first P frame of a process -- of a closed GOP
 * under the per-GOP parity definition; a context starts there), updated to the state after it, to be carried to the next frame
 * exactly as the reference's own extractor process carries it -- also by a call that returns PCAMV_EUNSUP because a sub-matrix would be
 * wider than 256 columns: the embedder draws the shorter one (width 256) before the longer one fails, and so does this.
 * pcamv_gpu_stc_extract = the same with lcg == NULL: tabulated widths only, PCAMV_EUNSUP otherwise. */
int pcamv_gpu_stc_extract(const uint8_t *stego, int n, int m, int matrixheight, uint8_t *message);
int pcamv_gpu_stc_extract_lcg(const uint8_t *stego, int n, int m, int matrixheight, int64_t *lcg, uint8_t *message);

/* H.264 MV-syntax extractor, the decode side of the BER check (the reference has none): parses the slice data
 * of a CABAC-coded P slice -- the bytes from the first macroblock's mb_skip_flag on, i.e. after the slice header and its
 * cabac_alignment bits, as encoder/cabac.c writes them (arithmetic decoding engine, mb_skip_flag, mb_type, sub_mb_type, mvd,
 * coded_block_pattern, mb_qp_delta, the residual, end_of_slice_flag) -- and returns every macroblock's i_type, i_partition,
 * i_sub_partition, ref[] and mv[] (MV prediction of H.264 8.4.1; P_SKIP inferred) in the record's layout; the other members are 0.
 * Host code, no GPU needed.  Scope: what the P slices of this path contain (frame macroblocks, one reference so no ref_idx,
 * 4x4 transform, cabac_init_idc 0): PCAMV_EUNSUP for an intra macroblock, PCAMV_EINVAL for a stream that does not end with
 * the picture's last macroblock.  The carrier LSBs of the result go to pcamv_gpu_stc_extract*. */
int pcamv_gpu_parse_pslice_cabac(const uint8_t *slice_data, size_t len, int mb_w, int mb_h, int slice_qp, pcamv_mb_t *out_mb);
/* the same for a CAVLC-coded P slice (--no-cabac): slice_data = from the first mb_skip_run to the rbsp trailing bits, as
 * encoder/cavlc.c writes them (mb_skip_run, mb_type, sub_mb_type, mvd, coded_block_pattern, mb_qp_delta, residual_block_cavlc) */
int pcamv_gpu_parse_pslice_cavlc(const uint8_t *slice_data, size_t len, int mb_w, int mb_h, pcamv_mb_t *out_mb);
/* The same on what a stream really holds.  pcamv_gpu_nal_to_rbsp undoes x264_nal_encode (common/common.c:658-690): optional Annex-B
 * start code, the NAL header byte (returned), emulation_prevention_three_bytes removed; rbsp must hold len bytes.  The _at forms
 * start at bit start_bit of the RBSP, i.e. right behind a slice header of any length (pcamv_gpu_parse_slice_header below reads
 * one, given what it needs of the SPS / PPS in use): CAVLC slice data begins at that bit, CABAC slice data after the
 * cabac_alignment_one_bits that fill up the byte. */
int pcamv_gpu_nal_to_rbsp(const uint8_t *nal, size_t len, uint8_t *rbsp, size_t *rbsp_len, int *nal_ref_idc, int *nal_unit_type);
int pcamv_gpu_parse_pslice_cabac_at(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, int slice_qp, pcamv_mb_t *out_mb);
int pcamv_gpu_parse_pslice_cavlc_at(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, pcamv_mb_t *out_mb);
/* The layer above a unit, host code: an Annex B byte stream cut into its NAL units.  A start code prefix is any 00 00 01; unit i
 * begins behind the i-th prefix and ends in front of the next one, or at len, without its trailing 00 bytes (trailing_zero_8bits, or
 * the zero_byte of a long start code).  Bytes in front of the first prefix belong to no unit; a unit may be empty (len 0,
 * nal_header -1).  off counts from bytes[0]; nal_header is the unit's first byte; kind comes from nal_unit_type and, for type 1, from
 * the first payload byte alone (its first bit is first_mb_in_slice == 0, slice_type is the ue behind it; emulation prevention cannot
 * touch that byte):
 *   PCAMV_UNIT_PSLICE  type 1, first_mb_in_slice 0, slice_type 0 or 5
 *   PCAMV_UNIT_UNSUP   type 1 with first_mb_in_slice != 0 (a second slice of a picture), slice_type B / SP / SI or none there is, or
 *                      without a payload byte; types 2, 3, 4 (data partitions)
 *   PCAMV_UNIT_OTHER   everything else: parameter sets, SEI, delimiters, IDR units, a type-1 I slice (it carries nothing)
 * forbidden_zero_bit is not judged here (pcamv_gpu_nal_to_rbsp fails such a unit).  units[cap] receives the first cap units,
 * *n_units counts all of them, *n_slices the stream's "slice units": those of kind PSLICE or UNSUP, in stream order. */
enum { PCAMV_UNIT_OTHER = 0, PCAMV_UNIT_PSLICE = 1, PCAMV_UNIT_UNSUP = 2 };
typedef struct pcamv_unit_t { int64_t off, len; int32_t nal_header, kind; } pcamv_unit_t;
int pcamv_gpu_annexb_index(const uint8_t *bytes, size_t len, pcamv_unit_t *units, size_t cap, int64_t *n_units, int64_t *n_slices);
/* What slice_header() (7.3.3) needs of the active SPS / PPS: the host's control plane, filled in by the caller.  Assumed beyond it:
 * frame_mbs_only_flag 1, one slice group.  log2_* 4 .. 16, poc_type 0 .. 2, num_ref_idx_l0_default (the count, not minus 1) 1 .. 32,
 * pic_init_qp 0 .. 51 (26 + pic_init_qp_minus26), pps_id 0 .. 255; anything else is PCAMV_EINVAL for every header. */
typedef struct pcamv_stream_params_t {
    int32_t log2_max_frame_num, poc_type, log2_max_poc_lsb, delta_pic_order_always_zero, pic_order_present, redundant_pic_cnt_present;
    int32_t num_ref_idx_l0_default, weighted_pred, entropy_cabac, pic_init_qp, deblocking_filter_control_present, pps_id;
} pcamv_stream_params_t;
/* The header of a P slice as x264_slice_header_write writes it (encoder/encoder.c:174-305), host code: rbsp[0, len) is the unit
 * behind its header byte, unescaped (pcamv_gpu_nal_to_rbsp).  *start_bit: the bit behind the header, the number the *_at calls take
 * (cabac_alignment_one_bits stay the parser's); *slice_qp = pic_init_qp + slice_qp_delta; *frame_num.  All three are -1 on failure.
 * In syntax order: nal_unit_type != 1, first_mb_in_slice != 0, slice_type not 0 or 5, pps_id != params->pps_id: PCAMV_EUNSUP;
 * frame_num; the POC fields of poc_type 0 / 1 / 2; redundant_pic_cnt; num_ref_idx_active_override_flag and its ue -- more than one
 * active reference, by it or by the default: EUNSUP; ref_pic_list_reordering walked to its 3 -- an idc above 3: PCAMV_EINVAL;
 * weighted_pred set: EUNSUP; with nal_ref_idc != 0 adaptive_ref_pic_marking_mode_flag 1: EUNSUP; with entropy_cabac cabac_init_idc
 * != 0: EUNSUP; slice_qp_delta -- a QP outside 0 .. 51: EINVAL; with deblocking control the idc (above 2: EINVAL) and its offsets.
 * A ue with more than 31 leading zeros, a read at or past bit 8 * len, and a start_bit at or past the end are EINVAL, found before
 * the element is judged.  Nothing outside rbsp[0, len) is read. */
int pcamv_gpu_parse_slice_header(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                 int32_t *slice_qp, int32_t *frame_num);

/* Device-resident variants used by bench.py and the multi-frame pipeline: planes are raw
 * device pointers (hipMalloc / torch storage), tightly packed like recon[] above.
 * set_ref_device takes effect with the plane production of the next step: a pass2_pframe before that step still
 * runs against the reference before (the second pass reads the produced planes only), first-pass pixels included.
 * set_fenc_device takes effect at once, like upload_fenc: a pass 2 that follows encodes every macroblock on it. */
int pcamv_gpu_set_ref_device(pcamv_ctx_t *ctx, const void *y, const void *u, const void *v,
                             const void *prev_mv, const void *prev_ref);
/* pass as prev_mv and prev_ref to chain frames on the device: the temporal candidates then come
 * from the motion field the context's previous step produced (kept in a ping-pong buffer) */
#define PCAMV_PREV_FIELD_INTERNAL ((const void *)(uintptr_t)1)
int pcamv_gpu_set_fenc_device(pcamv_ctx_t *ctx, const void *y, const void *u, const void *v);
/* One full step on resident inputs: plane production + analysis + RCA + embedding; results
 * stay on the device until pcamv_gpu_fetch_results. stream = hipStream_t as void*. */
int pcamv_gpu_step_device(pcamv_ctx_t *ctx, int qp, float emrate, void *stream);
int pcamv_gpu_fetch_results(pcamv_ctx_t *ctx, pcamv_mb_t *out_mb, pcamv_embed_t *out);
/* Batches: several contexts (independent closed GOPs of the same size on the same device) advance
 * one frame per step together; every kernel launch then carries the same dependency step of all
 * of them.  A single 1080p frame exposes at most 60 independent macroblocks at a time,
 * the batch is what fills the 256 CUs.  The contexts keep their own inputs/outputs (set_ref_device,
 * set_fenc_device, fetch_results); the batch only owns the launch descriptors and the scheduler
 * state; destroy a batch before closing its contexts.
 * Scheduling of the analysis inside a step: by default ONE persistent launch ("k_analyse_flow") in
 * which ready macroblocks of all GOPs flow through a device queue (search -> publish motion ->
 * RCA costs -> reconstruction per macroblock); with PCAMV_SCHED=diag in the environment at
 * batch/context creation, one launch per anti-diagonal ("k_search_diag") followed by RCA and
 * reconstruction launches.  Results are identical; kernel_time takes the name of the active one.
 * The closed loop's second pass (pass 2 + loop filter) follows the same choice: one persistent launch
 * ("k_pass2_deblock_flow") through the same queue, or one launch per anti-diagonal. */
int  pcamv_gpu_batch_create(pcamv_ctx_t *const *ctxs, int n, pcamv_batch_t **batch);
void pcamv_gpu_batch_destroy(pcamv_batch_t *batch);
int  pcamv_gpu_batch_step(pcamv_batch_t *batch, int qp, float emrate, void *stream);
/* The time of one of the batch's timed kernels: the average over its launches since the last reset, and their number.  Synchronises.
 * kernel: the dominant kernel's name (pcamv_gpu_batch_dominant_kernel, below), or one of the 40 that follow -- the list the library
 * keeps as PCAMV_TIMERS in csrc/pcamv_gpu.hip; any other name is PCAMV_EINVAL:
 *   the embedding and the receiving side: "k_embed_prepare", "k_extract_prepare", "k_extract_bits", "k_payload_check",
 *     "k_extract_count", "k_extract_chain";
 *   slices and NAL units: "k_parse_pslice", "k_parse_pslice_cavlc", "k_write_pslice", "k_write_pslice_cavlc", "k_nal_to_rbsp";
 *   byte streams received: "k_stream_plan", "k_stream_scan", "k_stream_prefix" (with the three kernels of a video's prefix),
 *     "k_stream_place", "k_stream_unit", "k_slice_header", "k_slice_header_sets", "k_stream_status", "k_stream_window_unit",
 *     "k_pset_unit", "k_pset_parse", "k_pset_resolve", "k_video_cut";
 *   byte streams written: "k_stream_open", "k_stream_open_heads", "k_stream_slot", "k_stream_commit", "k_stream_join",
 *     "k_stream_copy_plan", "k_stream_copy", "k_idr_mb", "k_idr_prefix", "k_idr_pack", "k_idr_unit";
 *   one message for the batch: "k_message_count", "k_message_plan", "k_message_jobs", "k_extract_chain_message",
 *     "k_message_check" (the two kernels of a check under one timer) */
int  pcamv_gpu_batch_kernel_time(pcamv_batch_t *batch, const char *kernel, double *avg_ms, int *launches, int reset);
/* ... and, the 41st of PCAMV_TIMERS, with PCAMV_FEATURE_IDR_DEBLOCK among the byte streams written: "k_idr_deblock", the loop filter of
 * the IDR pictures -- its average is per launch, and a call launches it once per anti-diagonal x + 2 y of the picture, mb_w + 2 (mb_h - 1)
 * times.  (Listed here and not above: tests/test_gpu_batch_memory.py counts the 40 of the list above.)
 * With PCAMV_FEATURE_IDR_SLICES, the 42nd and 43rd: "k_idr_unit_len", one wavefront per (context, slice) counting its unit's bytes, and
 * "k_idr_place", one lane per context placing its units; both are launched only for pictures of more than one slice, for which
 * "k_idr_prefix", "k_idr_pack" and "k_idr_unit" time the kernels that work per slice.
 * With PCAMV_FEATURE_IDR_I4X4, the 44th: "k_idr_mb4", which stands in k_idr_mb's place in a call with i4x4 != 0 -- its average is per
 * launch, and such a call launches it once per anti-diagonal x + 2 y of the picture.
 * With PCAMV_FEATURE_RATE, the 45th and 46th: "k_frame_qp", one wavefront per context putting the row of the context's QP in force into
 * the descriptor just pushed -- launched behind a descriptor upload only while some context of the batch has a QP in force on the
 * device --, and "k_rate_update", one lane per context, behind k_stream_commit while a rate is open.
 * With PCAMV_FEATURE_SOURCE, the 47th: "k_source_feed", one launch per pcamv_gpu_batch_feed_device call and none otherwise. */
const char *pcamv_gpu_batch_last_error(const pcamv_batch_t *batch);
/* Closed loop on the device: with on != 0 every batch step ends with pass 2 + the loop filter (embedding must be
 * on: the flip map comes from it), leaving each context's deblocked reconstruction in its device planes
 * (pcamv_gpu_recon_device) -- hand those to set_ref_device as the next frame's reference. */
int  pcamv_gpu_batch_set_closed_loop(pcamv_batch_t *batch, int on);
int  pcamv_gpu_recon_device(pcamv_ctx_t *ctx, void *planes[3]);
/* host copy of those planes (tightly packed w*h, w/2*h/2 x2) after synchronising */
int  pcamv_gpu_fetch_recon(pcamv_ctx_t *ctx, uint8_t *const planes[3]);
/* name of the analysis kernel the batch's schedule launches ("k_analyse_flow", "k_analyse_flow_rd" with --subme >= 6,
 * "k_analyse_flow_tesa", or "k_search_diag") */
const char *pcamv_gpu_batch_dominant_kernel(const pcamv_batch_t *batch);
/* Results of the step enqueued last, for every context of the batch, copied on `stream` without synchronising the host:
 * context i's pass-1 records (n_mb x pcamv_mb_t) to (char *)dst_mb + i * mb_stride and, when dst_flip != NULL, its flip map
 * (16 * n_mb bytes, the first `n carriers` meaningful) to (char *)dst_flip + i * flip_stride.  The destinations may be device
 * memory or pinned host memory; the caller orders `stream` after the step's stream (an event) and owns the synchronisation.
 * This is what lets a host pipeline overlap a step's downloads with the next step (bench.py pcie_inclusive). */
int  pcamv_gpu_batch_copy_results_async(pcamv_batch_t *batch, void *dst_mb, size_t mb_stride, void *dst_flip, size_t flip_stride, void *stream);

/* Average duration in ms of the dominant kernel over the launches since the last reset,
 * measured with hipEvents on the launch stream (bench.py roofline). */
int pcamv_gpu_kernel_time(pcamv_ctx_t *ctx, const char *kernel, double *avg_ms, int *launches, int reset);

/* Pixel-metric probe for parity tests of the cost functions themselves (common/pixel.c SAD/SATD,
 * common/mc.c get_ref / mc_chroma): n requests {mb_x, mb_y, i_pixel, xoff, yoff, mvx, mvy (qpel),
 * satd}, each answered with {luma cost, U cost, V cost} of the uploaded fenc block against the
 * current reference at that MV (no MV-bit cost added).  qp is the probe's own: the context keeps the QP of its
 * last analysis or step, and pass 2, the embedding stage, the writers and the next analysis behave as if the probe
 * had not happened (the context's table for qp is made on first use and kept). */
int pcamv_gpu_block_costs(pcamv_ctx_t *ctx, int qp, int n, const int32_t *req, int32_t *out);

/* Probe of the RD stage's metrics and intra predictors on caller-supplied pixels, for parity tests against reference-minted vectors
 * (common/pixel.c:71-96 ssd, :256-358 sa8d / hadamard_ac; encoder/rdo.c:106-137 ssd_mb with the psy-RD term; encoder/analyse.c:522-549
 * x264_mb_cache_fenc_satd; common/predict.c 16x16 / chroma 8x8 / 4x4 predictors scored with satd -- sad at subme 1 -- as the intra
 * analysis of analyse.c:552-879 does).  n requests of 1024 bytes: source macroblock (Y 16x16 rows of 16, then 8 rows of U | V),
 * a second macroblock in the same layout, intra borders top[3][28] ([c][3] = top-left sample, [c][4 + x]; luma 24 wide) and
 * left[3][16], int32 avail at byte 900 (bit 0 left, bit 1 top).  out: 32 int32 per request -- 0 ssd 16x16 + 2 x 8x8 of source vs
 * second block, 1 the same + the psy term (ssd_mb), 2 / 3 hadamard_ac 16x16 of the second block's luma (4x4 / 8x8 energies),
 * 4 / 5 fenc_satd_sum / fenc_sa8d_sum of the source, 6..9 intra 16x16 V, H, DC (variant by avail), P, 10..13 intra chroma DC
 * (variant), H, V, P over both planes, 14..25 the twelve 4x4 modes on block 0 (x264's I_PRED_4x4 order); unavailable = 1 << 28.
 * Like pcamv_gpu_block_costs it leaves the context as it found it: qp, and the slice-start context states that go with it, are the probe's own. */
int pcamv_gpu_rd_probe(pcamv_ctx_t *ctx, int qp, int n, const uint8_t *req, int32_t *out);

/* Probe of the embedding stage on a caller's records, for parity tests of the cover / cost assembly and the syndrome-trellis kernels
 * at inputs no analysis produces: mbs[mb_count] is copied into the context's record buffer, then the stage runs exactly as
 * pcamv_gpu_embed_pframe runs it (same kernels and outputs; the rand() stream, the payload cursor and the column generator move the
 * same way).  Afterwards the context stands as after an analysis that produced those records: pcamv_gpu_final_mvs,
 * pcamv_gpu_batch_extract_step and the slice writers' final motion see them and the new flip map; pcamv_gpu_pass2_pframe encodes
 * every macroblock of them (the reconstruction planes hold no first pass of these records).  Synchronises. */
int pcamv_gpu_embed_records(pcamv_ctx_t *ctx, const pcamv_mb_t *mbs, float emrate,
                            const uint8_t *message, int message_len, pcamv_embed_t *out);

/* Diagnostics: record every block-cost evaluation {ip,xoff,yoff,mvx,mvy,flags,cost,cost2} made for
 * macroblock mb by the next analyse call (mb < 0: off); out holds 1 + 8*4000 int32, out[0] = count. */
int pcamv_gpu_trace_mb(pcamv_ctx_t *ctx, int mb);
int pcamv_gpu_trace_fetch(pcamv_ctx_t *ctx, int32_t *out);

/* Diagnostics for the parity tests of the RD mode decision (--subme >= 6 with CABAC): FNV-1a of the 460 context states
 * after every macroblock of the following analyses; out holds mb_count words. */
int pcamv_gpu_debug_state_hash(pcamv_ctx_t *ctx, int enable);
int pcamv_gpu_debug_state_hash_fetch(pcamv_ctx_t *ctx, uint32_t *out);

int pcamv_gpu_abi_version(void);
/* What the library can do beyond the calls of its ABI version: a mask of PCAMV_FEATURE_* (additions keep the version). */
#define PCAMV_FEATURE_PAYLOAD 0x1u      /* the payload path below */
#define PCAMV_FEATURE_SLICE_PARSER 0x2u /* CABAC P slices parsed on the device (the receiver from a stream, at the end of this file) */
#define PCAMV_FEATURE_SLICE_PARSER_CAVLC 0x4u   /* ... and CAVLC P slices (the *_cavlc calls there) */
#define PCAMV_FEATURE_SLICE_WRITER 0x8u /* CABAC P slices written on the device (the sender to a stream, at the end of this file) */
#define PCAMV_FEATURE_SLICE_WRITER_CAVLC 0x10u  /* ... and CAVLC P slices (the *_cavlc calls there) */
#define PCAMV_FEATURE_NAL_DEVICE 0x20u  /* the receiver takes NAL units: emulation prevention undone on the device (the *_nals* calls) */
#define PCAMV_FEATURE_STREAM_DEVICE 0x40u       /* the receiver takes Annex B byte streams: units found and slice headers read on the device */
#define PCAMV_FEATURE_STREAM_WRITER 0x80u       /* the sender writes Annex B byte streams: slice headers and unit placement on the device */
#define PCAMV_FEATURE_STREAM_WINDOW 0x100u      /* the receiver on byte streams takes a window of slice units per context in one call */
#define PCAMV_FEATURE_PARAM_SETS 0x200u        /* SPS / PPS read on the device, per stream: the *_param_sets and *_sets calls at the end of this file */
#define PCAMV_FEATURE_VIDEO 0x400u      /* one video of many chains: per-chain heads, streams joined, a video cut at its IDR units on the device */
#define PCAMV_FEATURE_MESSAGE 0x800u    /* one message for a batch, split over its contexts' frames on the device (behind the payload path below) */
#define PCAMV_FEATURE_IDR 0x1000u       /* the IDR picture a chain starts with coded on the device (the last section of this file) */
#define PCAMV_FEATURE_IDR_DEBLOCK 0x2000u       /* ... and filtered there, as the stream's P pictures are (the *2 calls of that section) */
#define PCAMV_FEATURE_IDR_SLICES 0x4000u        /* ... in several slices of whole macroblock rows, a wavefront per slice (the *3 calls of that section) */
#define PCAMV_FEATURE_IDR_I4X4 0x8000u          /* ... with Intra4x4 macroblocks beside the Intra16x16 ones (the *4 calls of that section, the decoders that end in 2) */
#define PCAMV_FEATURE_RATE 0x10000u     /* a QP per context, from the host or from device memory, and the rate controller on the device (the section on rate control at the end of this file) */
#define PCAMV_FEATURE_SOURCE 0x20000u   /* the sender takes a video: pictures of any even size fed to all contexts of a batch out of a clip in device memory, and parameter sets that say how to crop them (the last section of this file) */
unsigned pcamv_gpu_features(void);

/* ---- Payload path: the caller's bits through the device-resident entry points, and back out on the device ----
 *
 * Sender.  The reference takes every frame's message from rand() (encoder.c:1838-1840), and so do embed_pframe(message == NULL),
 * step_device and batch_step.  A payload attached to a context replaces that source: packed bytes, 8 bits per byte, most
 * significant bit first, n_bits long.  A frame that embeds m bits takes payload bits cursor .. cursor + m - 1 (zeros past the
 * payload's end) and the cursor -- a device word, so closed-loop steps need no host round trip although m is only known on the
 * device -- advances by m whatever stc_ok turns out to be, like the rand() stream does: a frame whose embedding failed costs its
 * own m bits and nothing after them, sender and receiver offsets stay aligned.  Attaching sets the cursor to 0.  While a payload
 * is attached the rand() state does not move; attaching NULL / 0 detaches, and the context embeds the rand() stream again from
 * where it stood.  An explicit `message` of pcamv_gpu_embed_pframe still wins and does not move the cursor.
 * set_payload copies host bytes; set_payload_device borrows a device buffer the caller keeps alive while attached.
 * payload_tell synchronises: bits consumed so far, bits of the attached payload. */
int pcamv_gpu_set_payload(pcamv_ctx_t *ctx, const uint8_t *bytes, int64_t n_bits);
int pcamv_gpu_set_payload_device(pcamv_ctx_t *ctx, const void *device_bytes, int64_t n_bits);
int pcamv_gpu_payload_tell(pcamv_ctx_t *ctx, int64_t *consumed_bits, int64_t *payload_bits);

/* Receiver (kernels k_extract_prepare, k_extract_bits; the reference has no extractor).  A frame's message is read
 * from its FINAL motion the way a decoder sees it: carriers in embedding order (encoder.c:1566-1647) of every coded macroblock
 * (i_type != PCAMV_P_SKIP), stego bit = LSB(mvx + mvy), m from n and emrate as the embedding stage computes it, the two
 * sub-matrices from a receive-side column generator of the context's own (initialised like the sender's, advanced the same way:
 * see pcamv_gpu_stc_extract_lcg), one thread per message bit.  The bits are packed like the payload and appended to the context's
 * received stream at a device-side write cursor that moves by m; a frame with m > n, or with sub-matrices that cannot be built,
 * appends m zero bits.
 * rx_reserve makes room for n_bits (0 releases) and empties the stream; rx_reset empties it (cursor 0, generator at its initial
 * state).  A frame that runs past the reservation sets a device flag, its bits beyond are dropped (nothing is written out of
 * bounds), and the next synchronising call of this group reports PCAMV_ENOMEM once.  rx_tell / rx_fetch synchronise. */
int pcamv_gpu_rx_reserve(pcamv_ctx_t *ctx, int64_t n_bits);
int pcamv_gpu_rx_reset(pcamv_ctx_t *ctx);
int pcamv_gpu_rx_tell(pcamv_ctx_t *ctx, int64_t *received_bits, int64_t *reserved_bits);
int pcamv_gpu_rx_fetch(pcamv_ctx_t *ctx, uint8_t *bytes, int64_t n_bits);
/* Every context's last step (its records and the flip map of its embedding stage, on the device: final MV = mv_stego where the map
 * says so, what pcamv_gpu_final_mvs returns) through the receiver, on `stream`, without a host synchronisation; call it after a
 * batch_step with the same emrate, between closed-loop steps or after the last.  Every context needs a reservation. */
int pcamv_gpu_batch_extract_step(pcamv_batch_t *batch, float emrate, void *stream);
/* One frame from host records that hold final motion (pcamv_gpu_parse_pslice_*): uploaded, same kernels.  bits_out (optional, room
 * for 16 * mb_count) receives the message bits one per byte, n / m (optional) the frame's carriers and message bits; with a
 * reservation the bits are appended to the received stream too.  Synchronises. */
int pcamv_gpu_extract_pframe(pcamv_ctx_t *ctx, const pcamv_mb_t *mbs, float emrate, uint8_t *bits_out, int32_t *n, int32_t *m);
/* diff[i] = number of bits in which context i's received stream differs from its attached payload, payload bits past its end
 * counting as zeros: the BER numerator of every chain from one kernel and one small copy.  Synchronises. */
int pcamv_gpu_batch_payload_check(pcamv_batch_t *batch, int64_t *diff);

/* ---- One message for one video: a batch-wide payload split on the device (PCAMV_FEATURE_MESSAGE) ----
 *
 * A payload belongs to one context, but a frame's message length m = frame_bits(emrate, n) is known only on the device, after that
 * frame's analysis: a caller with ONE message for the many chains of a video cannot split it beforehand.  A message attached to a
 * batch is split there.  The rule (csrc/pcamv_message.h is its definition, pcamv_gpu_message_plan its export without a GPU):
 *
 *   A job is one frame of one context in one call; a step call has k = 1 slot per context, a window call k.  The jobs of a call are
 *   ordered slot-major, context-minor: (w, i) before (w', i') iff w < w', or w == w' and i < i' -- a window of k is observationally
 *   k steps.  With the batch cursor B at the start of the call, job (w, i) owns the message bits at(w, i) .. at(w, i) + m(w, i) - 1,
 *   at(w, i) = B + the sum of m over the jobs before it, and afterwards B += the sum of m over all jobs.  A job of status 0
 *   contributes its m whatever stc_ok or the sub-matrices turn out to be (the per-context rule); PCAMV_EEOF contributes 0 bits and is
 *   no failure; any other status contributes 0 bits and is a failure: its m is unknown, so everything behind it is misaligned.
 *   Two sticky words: valid_bits = the smallest `at` of a failed job (received_bits while there is none), first_bad = that job's
 *   (calls since the reset before its own, w, i), -1 each while there is none.  Bits past the message's end are zeros on the sender;
 *   bits at or beyond the receiver's reservation are dropped, never written, and the next synchronising call of this group returns
 *   PCAMV_ENOMEM once (the rule of a context's stream).  The column generators stay per context on both sides, advanced in slot order.
 *
 * The contract between sender and receiver, next to the emrate contract: the receiving batch has the sender's context count,
 * context i takes GOP first_gop + i (pcamv_gpu_batch_index_video*), and rounds follow the sender's order.  A picture the sender
 * failed to write (pcamv_gpu_batch_write_status -3) still consumed its m bits, which no receiver can see: checking write_status stays
 * the caller's, as do error correction and the distribution of a message across GPUs.
 *
 * Sender.  set_message attaches packed bytes (copied; set_message_device borrows a device buffer) to the batch and sets the cursor to
 * start_bit, so that another batch -- a last, smaller round -- can continue a message; NULL / 0 detaches.  PCAMV_EINVAL if a member
 * context has a payload of its own (or belongs to another batch with a message).  While attached, pcamv_gpu_set_payload*,
 * pcamv_gpu_step_device and pcamv_gpu_embed_pframe(message == NULL) on a member return PCAMV_EINVAL; an explicit `message` still wins
 * and moves nothing.  Every batch_step with emrate > 0 then runs k_message_count (every context's n, m), k_message_plan (every
 * context's place, into its payload cursor) and the embedding stage as with a payload.  message_tell synchronises: the cursor, the
 * message's bits. */
int pcamv_gpu_batch_set_message(pcamv_batch_t *batch, const uint8_t *bytes, int64_t n_bits, int64_t start_bit);
int pcamv_gpu_batch_set_message_device(pcamv_batch_t *batch, const void *device_bytes, int64_t n_bits, int64_t start_bit);
int pcamv_gpu_batch_message_tell(pcamv_batch_t *batch, int64_t *next_bit, int64_t *n_bits);
/* Receiver.  rx_message_reserve makes room for n_bits of one received stream for the batch (0 releases) and empties it;
 * rx_message_reset empties it: cursor 0, the sticky words cleared, every member's column generator at its initial state.  While the
 * reservation exists every extract call of the batch (extract_step, extract_slices*, extract_nals*, extract_stream_step*,
 * extract_stream_window*, the *_sets forms) writes into it by the rule -- k_extract_count, k_message_jobs, k_message_plan,
 * k_extract_chain_message, k_extract_bits -- and the contexts need no reservation of their own: their streams and cursors do not
 * move.  slice_status, window_status and the stream cursors behave as without one.  The extract calls of a batch with a reservation
 * belong on one stream.  rx_message_tell / rx_message_fetch / message_check synchronise.  message_check: the number of bits in
 * which the received stream differs from the message attached to this batch over [0, min(received, reserved)), message bits past
 * its end counting as zeros. */
int pcamv_gpu_batch_rx_message_reserve(pcamv_batch_t *batch, int64_t n_bits);
int pcamv_gpu_batch_rx_message_reset(pcamv_batch_t *batch);
int pcamv_gpu_batch_rx_message_tell(pcamv_batch_t *batch, int64_t *received_bits, int64_t *reserved_bits, int64_t *valid_bits, int64_t first_bad[3]);
int pcamv_gpu_batch_rx_message_fetch(pcamv_batch_t *batch, uint8_t *bytes, int64_t n_bits);
int pcamv_gpu_batch_message_check(pcamv_batch_t *batch, int64_t *diff, int64_t *received_bits, int64_t *valid_bits);
/* (tests) synchronises; *guard_intact = are the guard words the library keeps behind the batch's received stream untouched */
int pcamv_gpu_batch_debug_rx_message_guard(pcamv_batch_t *batch, int *guard_intact);
/* The rule without a GPU.  m / status: [contexts * k], job i * k + w is slot w of context i (status NULL: all 0); capacity < 0: none.
 * state: PCAMV_MESSAGE_STATE_WORDS words -- [0] cursor, [1] smallest `at` of a failed job or -1, [2..4] first_bad, [5] overrun flag,
 * [6] calls so far -- made by message_state_reset, carried from call to call; at: [contexts * k] out.  message_frame_bits: m of a
 * frame with n carriers, as both sides compute it.  message_plan_device is the parity probe of k_message_plan: the same on the
 * device for the caller's arrays, no context's state involved; `at` has room for one word more, which comes back as the device
 * left it (bytes 0xA5 beforehand). */
#define PCAMV_MESSAGE_STATE_WORDS 8
void pcamv_gpu_message_state_reset(int64_t *state, int64_t cursor);
int32_t pcamv_gpu_message_frame_bits(float emrate, int32_t n_carriers);
int pcamv_gpu_message_plan(const int32_t *m, const int32_t *status, int contexts, int k, int64_t capacity, int64_t *state, int64_t *at);
int pcamv_gpu_message_plan_device(pcamv_ctx_t *ctx, const int32_t *m, const int32_t *status, int contexts, int k, int64_t capacity, int64_t *state, int64_t *at);

/* ---- Receiver from a stream: CABAC P slices parsed on the device (kernel k_parse_pslice, one wavefront per slice) ----
 *
 * What a receiver holds is a stream.  These calls take RBSP bytes (the *_nals* calls further down take NAL units; the caller gives the
 * bit behind the slice header and the slice QP, as for pcamv_gpu_parse_pslice_cabac_at) and parse them where the extractor runs: no
 * host parse, no upload of records, no synchronisation per frame.  Scope and return codes per slice are the host parser's: frame
 * macroblocks, one reference, 4x4 transform, cabac_init_idc 0; PCAMV_EUNSUP for an intra macroblock, PCAMV_EINVAL for a slice that
 * ends in the wrong place, runs out of bytes or has bad alignment bits.  The host parser is the independent check of this one
 * (tests/test_slice_parse_emu.py, test_slice_parse_fuzz.py, test_gpu_slice_parser.py).  A slice is at most 2^30 bytes.
 * The stream's entropy mode is stated by the call: these calls take CABAC slices and refuse contexts opened with b_cabac == 0 with
 * PCAMV_EUNSUP; --no-cabac streams go through the *_cavlc calls below.
 *
 * parse_pslice_cabac_device: the parity probe.  One slice from host bytes, parsed on the device, the mb_count records copied back;
 * the picture size is the context's.  Synchronises. */
int pcamv_gpu_parse_pslice_cabac_device(pcamv_ctx_t *ctx, const uint8_t *rbsp, size_t len, size_t start_bit, int slice_qp, pcamv_mb_t *out_mb);
/* One slice per context of the batch: staged into one device buffer with one copy on `stream`, parsed by one launch into every
 * context's receive-side records, then the receiver's kernels as in pcamv_gpu_batch_extract_step (the records hold final motion:
 * no flip map).  No host synchronisation: the bits are appended at each context's device-side cursor.  Every context needs a
 * reservation (pcamv_gpu_rx_reserve), else PCAMV_EINVAL.  A slice that fails to parse sets its context's status word on the
 * device and that context appends NOTHING in this call: cursor and receive-side column generator are untouched. */
typedef struct pcamv_slice_t { const uint8_t *rbsp; size_t len; size_t start_bit; int32_t slice_qp; } pcamv_slice_t;
int pcamv_gpu_batch_extract_slices(pcamv_batch_t *batch, const pcamv_slice_t *slices, float emrate, void *stream);
/* the same on bytes that are on the device already (a torch uint8 tensor, say): slice i is bytes[off[i] .. off[i] + len[i]) of a
 * borrowed buffer of bytes_size bytes; off / len / start_bit (int64) and slice_qp (int32) are device arrays of one entry per
 * context, kept alive and unchanged until the work queued on `stream` is done.  Entries that do not fit the buffer fail as
 * PCAMV_EINVAL slices; nothing outside it is read.
 * Ordering is the caller's.  The parser is queued on `stream` -- NULL: the first context's own stream, which is non-blocking and
 * waits for no other stream -- and reads the buffer and the arrays there: whatever produced them must be complete on that
 * stream's timeline before this call (produced on `stream` itself, `stream` made to wait for the producer's event, or a host
 * synchronisation), and nothing may rewrite them until the work queued here is done.  The library adds no synchronisation. */
int pcamv_gpu_batch_extract_slices_device(pcamv_batch_t *batch, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                          const int64_t *start_bit, const int32_t *slice_qp, float emrate, void *stream);
/* synchronises; status[i] = return code of context i's slice in the last extract_slices call (0, PCAMV_EINVAL or PCAMV_EUNSUP) */
int pcamv_gpu_batch_slice_status(pcamv_batch_t *batch, int32_t *status);
/* Diagnostics for the parity tests: the records the context's last slice parsed to (mb_count of them; synchronises), and whether
 * the guard region the library keeps behind that buffer still holds its pattern (*guard_intact, optional). */
int pcamv_gpu_debug_slice_records(pcamv_ctx_t *ctx, pcamv_mb_t *out_mb, int *guard_intact);

/* ---- The same for --no-cabac streams: CAVLC P slices parsed on the device (kernel k_parse_pslice_cavlc, one wavefront per slice) ----
 *
 * What changes is the syntax read (mb_skip_run, Exp-Golomb header, residual_block_cavlc, rbsp_slice_trailing_bits) and that there is
 * no slice QP: the slice data begins at bit start_bit of the RBSP, which need not be a byte boundary, as for
 * pcamv_gpu_parse_pslice_cavlc_at.  Return codes per slice are that host parser's on every input: PCAMV_EUNSUP for an intra
 * macroblock, PCAMV_EINVAL for a code no table has, a slice whose bits run out or are left over, or a start bit at or behind the
 * end (tests/test_slice_parse_cavlc_emu.py, test_slice_parse_cavlc_fuzz.py, test_gpu_slice_parser_cavlc.py).
 * These calls require contexts opened with b_cabac == 0 and refuse CABAC contexts with PCAMV_EUNSUP (those go through the calls
 * above).  Everything else is shared with them: staging with one copy, borrowed device buffers and their ordering rule, the
 * per-context status (pcamv_gpu_batch_slice_status), pcamv_gpu_debug_slice_records and its guard, a failed slice appending nothing,
 * no host synchronisation. */
int pcamv_gpu_parse_pslice_cavlc_device(pcamv_ctx_t *ctx, const uint8_t *rbsp, size_t len, size_t start_bit, pcamv_mb_t *out_mb);
int pcamv_gpu_batch_extract_slices_cavlc(pcamv_batch_t *batch, const pcamv_slice_t *slices, float emrate, void *stream);      /* slice_qp is not read */
int pcamv_gpu_batch_extract_slices_cavlc_device(pcamv_batch_t *batch, const void *bytes, size_t bytes_size, const int64_t *off,
                                                const int64_t *len, const int64_t *start_bit, float emrate, void *stream);

/* ---- The receiver on NAL units: emulation prevention undone on the device (kernel k_nal_to_rbsp, one wavefront per unit) ----
 *
 * The extract_slices* calls above with NAL units in place of RBSPs -- what a stream carries and what the writers below produce with
 * as_nal = 1: optional Annex B start code (long or short), header byte, payload with emulation_prevention_three_bytes.  One launch of
 * k_nal_to_rbsp in front of the parser undoes that layer for every context's unit, with the semantics of pcamv_gpu_nal_to_rbsp on every
 * input: a unit with nothing behind its start code, with forbidden_zero_bit set, with 00 00 0{0,1,2} behind its header byte or with
 * 00 00 03 xx, xx > 03, is a PCAMV_EINVAL slice (it appends nothing; pcamv_gpu_batch_slice_status); nal_unit_type is not looked at.
 * The RBSPs go to a buffer of the library's, taken in turn with a second one like the staging buffers: the caller's bytes are read
 * only.  One unit per context per call.
 * start_bit counts bits of the RBSP, from the first byte behind the NAL header byte: the number the RBSP calls take.  The units of
 * one call must not overlap one another in `bytes`: unit i's RBSP is written at [off[i], off[i] + len[i]) of the library's buffer, so
 * an overlap is never a memory error, but what overlapping units unescape to is unspecified.
 * nal_header (optional): an int32 device array of one entry per context that receives each unit's header byte, -1 for a unit
 * without one; it belongs to `stream` like the other arrays.  Borrowed buffers and their ordering rule, staging with one copy, the
 * refusal of the other entropy mode's contexts (PCAMV_EUNSUP) and the per-context status are those of the calls above. */
int pcamv_gpu_batch_extract_nals(pcamv_batch_t *batch, const pcamv_slice_t *units, float emrate, void *stream);        /* rbsp / len: the unit */
int pcamv_gpu_batch_extract_nals_cavlc(pcamv_batch_t *batch, const pcamv_slice_t *units, float emrate, void *stream);
int pcamv_gpu_batch_extract_nals_device(pcamv_batch_t *batch, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                        const int64_t *start_bit, const int32_t *slice_qp, int32_t *nal_header, float emrate, void *stream);
int pcamv_gpu_batch_extract_nals_cavlc_device(pcamv_batch_t *batch, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                              const int64_t *start_bit, int32_t *nal_header, float emrate, void *stream);
/* The parity probe; synchronises.  n units of one host buffer, unit i at bytes[off[i] .. off[i] + len[i]), unescaped by one launch on
 * the context's device and stream (nothing else of the context is used).  out[bytes_size] receives unit i's RBSP at off[i] and is
 * otherwise returned as it came (a caller's guard pattern survives); out_len[i] its length or -1, status[i] its return code,
 * nal_header[i] (optional) its header byte or -1.  Entries that do not fit the buffer are PCAMV_EINVAL units. */
int pcamv_gpu_nal_to_rbsp_device(pcamv_ctx_t *ctx, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                 uint8_t *out, int64_t *out_len, int32_t *status, int32_t *nal_header);

/* ---- The receiver on byte streams: NAL units found and slice headers read on the device ----
 *
 * What a receiver really has: one Annex B byte stream per chain -- start codes, parameter sets, SEI, delimiters, an IDR picture, then
 * P slices whose headers carry frame_num, the POC bits and slice_qp_delta.  index_streams cuts every context's stream into its units
 * once; extract_stream_step then feeds one slice unit per context and call through unescape -> header -> parse -> extract with no host
 * synchronisation and no per-frame array from the caller.  The semantics are those of pcamv_gpu_annexb_index and
 * pcamv_gpu_parse_slice_header on every input.
 *
 * The scan is data-parallel over bytes: a wavefront takes one chunk of PCAMV_STREAM_CHUNK bytes of one stream (k_stream_scan: the
 * prefixes and slice units a chunk starts, its last non-zero byte and last prefix), one wavefront per stream makes the exclusive prefix
 * over its chunks (k_stream_prefix), and a second scan writes every unit at its place (k_stream_place): nothing depends on the order
 * in which wavefronts finish.  Each context's table keeps its first max_units slice units (kinds PSLICE and UNSUP, in stream order);
 * the count returned is the full count.
 *
 * index_streams_device: context i's stream is bytes[off[i] .. off[i] + len[i]) of a borrowed device buffer; off / len are device int64
 * arrays of one entry per context, read by this call alone (the library keeps its own copy).  The streams of one call must not
 * overlap: the library's working memory is sized for bytes_size bytes in all, and a stream that no longer fits it gets n_slices_out
 * PCAMV_EINVAL (like one that does not fit the buffer) and an empty table; every step of such a context is PCAMV_EINVAL too, and
 * stream_tell gives its total as PCAMV_EINVAL.  The call builds the tables, sets every context's unit
 * cursor to 0, synchronises ONCE, returns each context's slice-unit count in n_slices_out[i] (host, optional) and sizes the RBSP slots
 * of the steps by the longest slice unit of the tables -- not by bytes_size.  The buffer stays borrowed until the next index call;
 * ordering on `stream` is the caller's, as for pcamv_gpu_batch_extract_slices_device.  Handing over complete units is the caller's
 * job: a stream cut inside a unit ends in a unit that fails in its step.  index_streams: the same from host bytes, one copy.
 *
 * extract_stream_step, for every context: the slice unit at the cursor is taken and the cursor moves on by one, whatever then happens
 * to the unit; a table at its end (or at max_units) gives PCAMV_EEOF and the cursor stays; a unit of kind UNSUP gives PCAMV_EUNSUP;
 * else the unit is unescaped (k_stream_unit, the control code of k_nal_to_rbsp), its header is read with `params` (k_slice_header:
 * start_bit and slice QP go where the parser reads them), it is parsed and extracted as by the *_nals* calls.  A context whose unit
 * failed at any stage appends nothing.  pcamv_gpu_batch_slice_status reports the code of the first stage that failed.
 * params->entropy_cabac chooses the parser; contexts of the other mode are refused with PCAMV_EUNSUP before anything is queued.
 * Before any index call: PCAMV_EINVAL.  nal_header (optional): device int32 array, one per context, receives the unit's header byte
 * (-1 where no unit was taken).  stream_tell synchronises: next[i] the cursor = slice units taken so far (a failed take at the end
 * does not count), total[i] the slice units of the stream. */
#define PCAMV_STREAM_CHUNK 2048
int pcamv_gpu_stream_chunk(void);               /* PCAMV_STREAM_CHUNK of the library in use */
int pcamv_gpu_batch_index_streams_device(pcamv_batch_t *batch, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                         int64_t max_units, int64_t *n_slices_out, void *stream);
typedef struct pcamv_stream_t { const uint8_t *bytes; size_t len; } pcamv_stream_t;
int pcamv_gpu_batch_index_streams(pcamv_batch_t *batch, const pcamv_stream_t *streams, int64_t max_units, int64_t *n_slices_out, void *stream);
int pcamv_gpu_batch_extract_stream_step(pcamv_batch_t *batch, const pcamv_stream_params_t *params, float emrate, int32_t *nal_header, void *stream);
int pcamv_gpu_batch_stream_tell(pcamv_batch_t *batch, int64_t *next, int64_t *total);
/* A window of slice units per context in one call (PCAMV_FEATURE_STREAM_WINDOW).  A slice is one serial chain on one wavefront, so a
 * step costs the latency of one slice however few contexts the batch has; the frames of one stream are independent in everything that
 * is expensive (a P slice parses on its own; carriers, stego bits and n of a frame depend on its records alone), and only the write
 * cursor of the received stream and the receiver's column generator chain from frame to frame, both cheap once every frame's n is
 * known.  So k units per context go through unescape (k_stream_window_unit), header, parser and carrier scan (k_extract_count) as
 * n * k independent jobs, one lane per context then walks its k slots in order (k_extract_chain), and k_extract_bits writes all of
 * them.  The rule: a window call of k is observationally k extract_stream_step calls.
 *
 * stream_window(k), 1 <= k <= PCAMV_STREAM_WINDOW_MAX, reserves per context x slot what a step keeps per context: receive-side records
 * (with the guard behind them), stego, hdr, cols, a status word, a row-scratch slot where the picture is wider than the parser's LDS
 * limit, and an RBSP slot sized as the index call sizes the steps'.  The memory is k times the step path's and k is the caller's
 * choice: a 1080p slot is about 2 MB (8160 records of 236 bytes, 128 KB of stego bytes), so 256 contexts x 8 slots take 4 GB.  k = 0
 * releases it.  The call synchronises and allocates, as an index call may; it belongs behind an index call (PCAMV_EINVAL before), and
 * an index call made later that needs longer RBSP slots regrows them.  The window call below never allocates.
 *
 * extract_stream_window(params, emrate, k): refused with PCAMV_EINVAL for k < 1 or k above the reserved count; every other refusal is
 * extract_stream_step's.  Slot w < k of context i takes the unit at cursor[i] + w if that lies within min(n_slices, max_units), else
 * its status is PCAMV_EEOF and it takes nothing; the cursor moves on by the number of slots that took a unit (a unit of kind UNSUP
 * counts as taken and gives PCAMV_EUNSUP; a context whose index failed gives PCAMV_EINVAL in every slot).  Each taken unit goes
 * through the step's stages with the step's codes.  Within a context the slots are appended to the received stream in slot order: a
 * slot with a non-zero status appends nothing and leaves write cursor and column generator where they were, the slots behind it go on
 * from there; m > n or sub-matrices that cannot be built append m zero bits and draw from the generator what a step draws; a slot
 * that runs past the reservation drops its bits beyond it and the next synchronising call reports PCAMV_ENOMEM once.  nal_header
 * (optional): device int32[n * k], context-major (i * k + w), the header byte or -1 where no unit was taken.  No host synchronisation
 * and no per-frame host arrays; a call waits on the device for the window call before it, whichever stream that was on.  Afterwards
 * pcamv_gpu_batch_slice_status returns slot k - 1's status of every context, pcamv_gpu_debug_slice_records the records of the last slot
 * that took a unit, stream_tell the cursor as moved: what k steps would have left.
 *
 * window_status synchronises: host int32[n * k] of the last window call, context-major. */
#define PCAMV_STREAM_WINDOW_MAX 64
int pcamv_gpu_batch_stream_window(pcamv_batch_t *batch, int k);
int pcamv_gpu_batch_extract_stream_window(pcamv_batch_t *batch, const pcamv_stream_params_t *params, float emrate, int k,
                                          int32_t *nal_header, void *stream);
int pcamv_gpu_batch_window_status(pcamv_batch_t *batch, int32_t *status);
/* The parity probes; they synchronise.  index_streams_probe: n streams of one host buffer through the three kernels, ALL units listed
 * (what pcamv_gpu_annexb_index lists).  units_out holds n tables of cap_per_stream + PCAMV_UNIT_GUARD entries each: the library fills
 * them with bytes 0xA5 on the device, the kernels write the first min(count, cap_per_stream) entries of each, and everything comes
 * back as the device left it (the guard entries behind a table must still hold the pattern).  n_units / n_slices: the full counts,
 * PCAMV_EINVAL for a stream that does not fit.  Fails with PCAMV_EHIP if the device copy of `bytes` was changed.
 * slice_headers_device: n RBSPs of one host buffer through k_slice_header, one lane each: rc / start_bit / slice_qp / frame_num as
 * pcamv_gpu_parse_slice_header gives them. */
#define PCAMV_UNIT_GUARD 4
int pcamv_gpu_index_streams_probe(pcamv_ctx_t *ctx, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                  pcamv_unit_t *units_out, int64_t cap_per_stream, int64_t *n_units, int64_t *n_slices);
int pcamv_gpu_slice_headers_device(pcamv_ctx_t *ctx, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                   const int32_t *nal_header, int n, const pcamv_stream_params_t *params, int32_t *rc, int64_t *start_bit,
                                   int32_t *slice_qp, int32_t *frame_num);

/* ---- Sender to a stream: CABAC P slices written on the device (kernel k_write_pslice, one wavefront per slice) ----
 *
 * A step leaves each context's final motion on the device (the records and the flip map); these calls turn it into the bytes a
 * receiver needs without a trip through the host: slice data as encoder/cabac.c writes it (cabac_init_idc 0, the states of the
 * slice QP, mb_qp_delta 0, one reference, 4x4 transform), the levels made again from the final motion with the step's source and
 * reference planes and the context's quantisers.  A P_SKIP macroblock's motion is inferred as a decoder infers it; a macroblock the
 * record calls coded is written as coded whatever it codes, since the receiver counts carriers per coded macroblock.
 * The slice header is the caller's, opaque here (its fields come from the SPS / PPS, the host's control plane): n_bits bits, most
 * significant first, behind which the writer puts cabac_alignment_one_bits and the slice data -- the RBSP form; with n_bits == 0
 * (or no header) the output is the bare slice data.  As a NAL unit: long start code, the header byte from nal_ref_idc and
 * nal_unit_type, the RBSP with emulation prevention as x264_nal_encode inserts it.  i_frame chooses the bit x264_cabac_encode_flush
 * takes from the frame counter (0x35a4e4f5 >> (i_frame & 31) & 1).
 * Contexts opened with b_cabac == 0 are refused with PCAMV_EUNSUP (they go through the *_cavlc calls below).  Several slices
 * per picture stay the host's (a chain's IDR picture: the last section of this file) (SPS and PPS: pcamv_gpu_param_set_head, the last section of this file); so does the slice header in these calls -- the stream calls at the end of this file make
 * it on the device. */
typedef struct pcamv_slice_hdr_t { const uint8_t *bits; int32_t n_bits; int32_t i_frame; int32_t nal_ref_idc; int32_t nal_unit_type; } pcamv_slice_hdr_t;
/* The parity probe; synchronises.  mbs == NULL: the context's last frame -- final == 0 the first-pass records as they are, final != 0
 * the records with the embedding stage's flip map (what the second pass reconstructed).  mbs != NULL: host records that hold final
 * motion already (what a parser returns), uploaded; only type, partition, sub-partition and mv are read.  hdr may be NULL (no header
 * bits, i_frame 0, nal_ref_idc 2, nal_unit_type 1).  out[cap] receives *len bytes; a slice that does not fit is PCAMV_ENOMEM. */
int pcamv_gpu_write_pslice(pcamv_ctx_t *ctx, const pcamv_slice_hdr_t *hdr, int final, const pcamv_mb_t *mbs, int as_nal, uint8_t *out, size_t cap, size_t *len);
/* Every context's last step with final motion, from one launch on `stream`, no host synchronisation.  hdrs: n_hdr == 1 (one header
 * for all contexts) or the batch size (NULL and 0: none), staged with one copy.  bytes is a borrowed device buffer of bytes_size
 * bytes; off and cap (in) and len (out) are device arrays of int64, one entry per context: slice i goes to bytes[off[i] .. off[i] +
 * cap[i]) and is len[i] long.  Nothing is written at or beyond a slice's capacity; a slice that does not fit sets its context's
 * status to PCAMV_ENOMEM and its len to 0.  With as_nal == 0, (bytes, off, len) is what pcamv_gpu_batch_extract_slices_device takes.
 * Ordering is the caller's, by the rule of that call; and this call belongs after the batch_step whose frame it writes and before the
 * next one, whose plane stage is the first thing to overwrite what the writer reads (that step's source planes, padded reference
 * planes, records and flip map). */
int pcamv_gpu_batch_write_step(pcamv_batch_t *batch, const pcamv_slice_hdr_t *hdrs, int n_hdr, int as_nal, void *bytes, size_t bytes_size,
                               const int64_t *off, const int64_t *cap, int64_t *len, void *stream);
/* synchronises; status[i] = 0 or PCAMV_ENOMEM for context i's slice of the last write call (PCAMV_EINVAL: its place is not inside the buffer) */
int pcamv_gpu_batch_write_status(pcamv_batch_t *batch, int32_t *status);
/* a capacity under which no slice of the context's picture size fails, for a header of hdr_bits bits, as RBSP or as a NAL unit */
int64_t pcamv_gpu_slice_bound(const pcamv_ctx_t *ctx, int32_t hdr_bits, int as_nal);
/* The same for contexts opened with --no-cabac (b_cabac = 0): CAVLC P slices, written by k_write_pslice_cavlc.  The slice data
 * follows the header's last bit directly (CAVLC has no alignment bits), hdr's i_frame is not read, and with as_nal = 0 the batch
 * call's (bytes, off, len) and the header's bit count are what pcamv_gpu_batch_extract_slices_cavlc_device takes as (bytes, off, len,
 * start_bit).  pcamv_gpu_batch_write_status and pcamv_gpu_slice_bound serve both modes.  Each pair of calls refuses the other entropy
 * mode's contexts with PCAMV_EUNSUP. */
int pcamv_gpu_write_pslice_cavlc(pcamv_ctx_t *ctx, const pcamv_slice_hdr_t *hdr, int final, const pcamv_mb_t *mbs, int as_nal, uint8_t *out, size_t cap,
                                 size_t *len);
int pcamv_gpu_batch_write_step_cavlc(pcamv_batch_t *batch, const pcamv_slice_hdr_t *hdrs, int n_hdr, int as_nal, void *bytes, size_t bytes_size,
                                     const int64_t *off, const int64_t *cap, int64_t *len, void *stream);
/* Host code, the inverse of pcamv_gpu_nal_to_rbsp: long start code, header byte, the RBSP with emulation prevention bytes as
 * x264_nal_encode inserts them (common/common.c:658-695).  nal[cap] receives *nal_len bytes (at most 5 + len + len / 2 + 1). */
int pcamv_gpu_rbsp_to_nal(const uint8_t *rbsp, size_t len, int nal_ref_idc, int nal_unit_type, uint8_t *nal, size_t cap, size_t *nal_len);

/* ---- The sender writes byte streams: slice headers written and units placed on the device ----
 *
 * The write_step* calls above take the slice header and every unit's place from the caller, per frame.  These calls need neither: a
 * batch is given one region of a device buffer per context once (stream_open), and every write_stream_step appends each context's last
 * step to its stream as [access unit delimiter +] P slice unit, the header made on the device from the step's QP, a picture counter
 * and the parameter sets.  Closed-loop contexts run step -> write_stream_step N times, then index_streams_device -> extract_stream_step
 * N times on the same (bytes, off, len): nothing per frame passes through the host on either side, and the bytes in between are a
 * well-formed Annex B stream.  SPS and PPS are written by pcamv_gpu_param_set_head and read by the *_param_sets calls (the last section of
 * this file).  A chain's IDR picture is written by pcamv_gpu_batch_write_stream_idr (the last section of this file), or stays the caller's
 * and goes into the stream's `head`, opaque here, behind the parameter sets.  Out of scope: several slices per picture.
 *
 * write_slice_header: host code, no GPU; the semantics of the device's header writer on every input (csrc/pcamv_stream_write.h), and the
 * inverse of pcamv_gpu_parse_slice_header.  slice_header() (7.3.3) of a P slice for `params`, element by element as
 * x264_slice_header_write emits it (encoder/encoder.c:174-305): first_mb_in_slice 0, slice_type, pps_id, frame_num, the POC elements of
 * poc_type (0: poc_lsb [, delta_pic_order_cnt_bottom]; 1 and not delta_pic_order_always_zero: delta_pic_order_cnt[0] [, [1]]; the second
 * of each with pic_order_present), redundant_pic_cnt if present, num_ref_idx_active_override_flag (0 if num_ref_idx_l0_default is 1, else
 * 1 and num_ref_idx_l0_active_minus1 = 0: the stream says one active reference), ref_pic_list_reordering_flag_l0 0,
 * adaptive_ref_pic_marking_mode_flag 0 if nal_ref_idc != 0, cabac_init_idc 0 with CABAC, slice_qp_delta = slice_qp - pic_init_qp, and
 * with deblocking control disable_deblocking_filter_idc and, unless it is 1, the two offsets.  bits[cap] receives (*n_bits + 7) / 8
 * bytes, most significant bit first, the last byte zero-filled: what pcamv_slice_hdr_t takes.  At most PCAMV_SLICE_HDR_MAX_BITS bits.
 * Refused before anything is written, every member judged whether `params` has its element written or not -- PCAMV_EINVAL: params
 * outside the ranges stated at pcamv_stream_params_t, frame_num or poc_lsb not below 2^log2_max_*, slice_qp outside 0 .. 51, slice_type
 * not 0 or 5, an idc outside 0 .. 2, an offset outside -6 .. 6, nal_ref_idc outside 0 .. 3, redundant_pic_cnt outside 0 .. 127, a POC
 * delta with |v| > 2^30 (the longest Exp-Golomb code the readers take); then PCAMV_EUNSUP: weighted_pred.  PCAMV_ENOMEM: cap too small. */
#define PCAMV_SLICE_HDR_MAX_BITS 215    /* derived in csrc/pcamv_stream_write.h */
#define PCAMV_SLICE_HDR_BYTES 28        /* a header's slot in the probe's output: the longest header, whole dwords */
typedef struct pcamv_slice_fields_t {
    int32_t nal_ref_idc, slice_type, frame_num, poc_lsb;
    int32_t delta_pic_order_cnt_bottom, delta_pic_order_cnt[2];
    int32_t redundant_pic_cnt, slice_qp;
    int32_t disable_deblocking_filter_idc;
    int32_t slice_alpha_c0_offset_div2, slice_beta_offset_div2;
} pcamv_slice_fields_t;
int pcamv_gpu_write_slice_header(const pcamv_stream_params_t *params, const pcamv_slice_fields_t *fields, uint8_t *bits, size_t cap, int32_t *n_bits);
/* What every picture of a batch's streams shares.  nal_ref_idc 1 .. 3 (0 is refused: in this path a chain's P frame is the next one's
 * reference); slice_type 0 or 5; first_pic >= 0; disable_deblocking_filter_idc 0 .. 2, or -1 for the reference's rule per picture
 * (encoder.c:159-169: 0 if 15 < qp + 2 * min(alpha, beta) of the two offsets below, else 1); aud 0 or 1.
 * Picture k of a stream (k = 0: the first write_stream_step after stream_open) has frame_num = (first_pic + k) mod 2^log2_max_frame_num,
 * poc_lsb = 2 (first_pic + k) mod 2^log2_max_poc_lsb, all POC deltas and redundant_pic_cnt 0 (encoder.c:1153-1158, 2282, 2306 for a
 * stream without B frames) and, for the CABAC writer's flush, i_frame = first_i_frame + k.
 * The three deblocking members are written as given and change nothing in the chain: a closed-loop step always runs the loop filter at
 * FilterOffsetA = FilterOffsetB = 0 and predicts the next picture from the filtered planes.  So only disable_deblocking_filter_idc -1, 0
 * or 2 with both offsets 0 describe what the chain predicts from, and only such a stream decodes to it (one slice per picture: 2 filters
 * as 0 does; -1 says 1 up to QP 15, where alpha and beta are 0 and the filter moves no sample).  With idc 1, or with an offset that is
 * not 0, a decoder reconstructs other pictures than the sender's and drifts (tests/test_gpu_pslice_decode.py). */
typedef struct pcamv_stream_write_t {
    int32_t nal_ref_idc, slice_type, first_pic, first_i_frame;
    int32_t disable_deblocking_filter_idc;
    int32_t slice_alpha_c0_offset_div2, slice_beta_offset_div2, aud;
} pcamv_stream_write_t;
/* stream_open: context i's stream is bytes[off[i] .. off[i] + cap[i]) of a borrowed device buffer of bytes_size bytes.  off / cap are
 * device int64 arrays of one entry per context, read by this call alone (the library keeps its own copy); len is a borrowed device int64
 * array that the library keeps current until the next open: len[i] = bytes of context i's stream so far, so that (bytes, off, len) is
 * at any time what pcamv_gpu_batch_index_streams_device takes.  head (optional: NULL / 0; host bytes, opaque, at most 2^24) -- the
 * caller's parameter sets and IDR picture -- is copied to the start of every stream (kernel k_stream_open, one lane per context, queued
 * on `stream`).  The call waits once for `stream`, for its copies of off, cap and head; the kernel is not waited for.  A context whose region does not lie inside the buffer, or does not hold head, gets len 0
 * and PCAMV_EINVAL in every step, and nothing is ever written for it.  The regions must not overlap.  params / wr out of range:
 * PCAMV_EINVAL, weighted_pred: PCAMV_EUNSUP, nothing is opened.
 *
 * write_stream_step follows write_step's ordering rule (after the batch_step it writes, before the next) and queues three launches on
 * `stream`, without host synchronisation: k_stream_slot, one lane per context (the picture's header into a header table of the
 * library's, the delimiter 00 00 00 01 09 30 at the stream's end if wr->aud, the place the writer gets; the QP is the step's, read from
 * the frame descriptor the writer reads it from), then k_write_pslice / k_write_pslice_cavlc unchanged with as_nal = 1 and that table,
 * then k_stream_commit, one lane per context.  params->entropy_cabac chooses the writer; contexts of the other mode are refused with
 * PCAMV_EUNSUP before anything is queued.  Before any open: PCAMV_EINVAL.
 * The picture counter moves on in every step for every context, whether the unit fits or not: a receiver sees the gap in frame_num.  The
 * delimiter and the unit succeed or fail together.  A picture that does not fit leaves the stream and len[i] where they were and sets
 * the context's status to PCAMV_ENOMEM (pcamv_gpu_batch_write_status serves: 0, PCAMV_ENOMEM, PCAMV_EINVAL); bytes between the stream's
 * end and the end of its region are then unspecified.  Nothing outside [off[i], off[i] + cap[i]) is ever written.
 * stream_written synchronises; each output is optional, one int64 per context: the stream's bytes (= len[i]), the steps since the open,
 * the slice units among them that are in the stream. */
int pcamv_gpu_batch_stream_open(pcamv_batch_t *batch, void *bytes, size_t bytes_size, const int64_t *off, const int64_t *cap, int64_t *len,
                                const pcamv_stream_params_t *params, const pcamv_stream_write_t *wr, const uint8_t *head, size_t head_len, void *stream);
int pcamv_gpu_batch_write_stream_step(pcamv_batch_t *batch, void *stream);
int pcamv_gpu_batch_stream_written(pcamv_batch_t *batch, int64_t *bytes, int64_t *pictures, int64_t *units);
/* The parity probe of the device's header writer; synchronises.  n cases, one parameter set and one pcamv_slice_fields_t per case, one
 * lane each (k_slice_headers_write): rc[i] and n_bits[i] as pcamv_gpu_write_slice_header gives them, the bits of case i in
 * bits[i * PCAMV_SLICE_HDR_BYTES ..), bytes of a slot behind a header's last byte 0. */
int pcamv_gpu_slice_headers_write_device(pcamv_ctx_t *ctx, const pcamv_stream_params_t *params, const pcamv_slice_fields_t *fields, int n,
                                         int32_t *rc, int32_t *n_bits, uint8_t *bits);

/* ---- Parameter sets: SPS / PPS read on the device, per stream (PCAMV_FEATURE_PARAM_SETS) ----
 *
 * The stream calls above take one pcamv_stream_params_t for the whole batch from the caller.  With these calls a receiver hands over
 * byte streams and nothing else: the units of nal_unit_type 7 and 8 of every context's stream are found, unescaped, parsed and resolved
 * on the device into one table per context, and the *_sets calls read each slice header under the entry its pps_id names.  The
 * contexts of a batch may come from different encoder configurations.  As everywhere here the host functions are the definition on
 * every input, valid or not.  Still the caller's: several slices per picture, parameter sets that change within a stream.
 *
 * parse_sps reads seq_parameter_set_data() (7.3.2.1) of rbsp[0, len) -- the unit behind its header byte, unescaped -- in syntax order:
 * profile_idc, the constraint byte, level_idc, sps_id; for profiles 100, 110, 122, 244, 44, 83, 86, 118, 128 chroma_format_idc, the two
 * bit depths, the transform bypass flag and seq_scaling_matrix_present_flag (else 1 / 8 / 8 / 0 / 0); log2_max_frame_num; poc_type and
 * its elements (type 1: the cycle is walked, its offsets are not kept); num_ref_frames, the gaps flag, width and height in macroblocks,
 * frame_mbs_only_flag, direct_8x8_inference_flag, the cropping flag and its four ue, vui_parameters_present_flag.  The VUI is not read.
 * parse_pps reads pic_parameter_set_rbsp() (7.3.2.2) through redundant_pic_cnt_present_flag and then, if more_rbsp_data(),
 * transform_8x8_mode_flag, pic_scaling_matrix_present_flag and second_chroma_qp_index_offset (has_tail 1; without a tail the second
 * offset is the first).  Data follows exactly if the read position lies before the last 1 bit of the RBSP; no 1 bit at or behind the
 * position is PCAMV_EINVAL.
 * The first failure in syntax order wins, and a read failure is found before the element is judged.  PCAMV_EINVAL: a read at or past
 * the end, a ue with more than 31 leading zeros, sps_id > 31, pps_id > 255, log2_*_minus4 > 12, poc_type > 2, a POC cycle > 255,
 * num_ref_idx_*_default_minus1 > 31, pic_init_qp_minus26 outside -26 .. 25, a chroma offset outside -12 .. 12, num_slice_groups_minus1
 * > 7, more than 2^16 macroblocks in either direction.  PCAMV_EUNSUP, at the element that says so: chroma_format_idc != 1, a bit depth
 * != 8, transform bypass, a sequence or picture scaling matrix, frame_mbs_only_flag 0, more than one slice group,
 * transform_8x8_mode_flag 1.  weighted_pred and a default of several references are not refused here: the slice-header reader judges
 * them per slice.  Elements without a range above are kept as the 32 bits read (num_ref_frames, the cropping offsets, pic_init_qs).
 * On failure *out is all zeros.  Members are values, not the coded "minus" forms: log2_* 4 .. 16 (log2_max_poc_lsb 0 where poc_type
 * is not 0), mb_w / mb_h counts, num_ref_idx_* counts, pic_init_qp / qs 26 + the coded value. */
typedef struct pcamv_sps_t {
    int32_t profile_idc, constraint_flags, level_idc, sps_id;
    int32_t chroma_format_idc, bit_depth_luma, bit_depth_chroma, transform_bypass, seq_scaling_matrix_present;
    int32_t log2_max_frame_num, poc_type, log2_max_poc_lsb, delta_pic_order_always_zero;
    int32_t offset_for_non_ref_pic, offset_for_top_to_bottom_field, num_ref_frames_in_poc_cycle;
    int32_t num_ref_frames, gaps_in_frame_num_allowed, mb_w, mb_h, frame_mbs_only, direct_8x8_inference;
    int32_t frame_cropping, crop_left, crop_right, crop_top, crop_bottom, vui_parameters_present;
} pcamv_sps_t;
typedef struct pcamv_pps_t {
    int32_t pps_id, sps_id, entropy_cabac, pic_order_present, num_slice_groups;
    int32_t num_ref_idx_l0_default, num_ref_idx_l1_default, weighted_pred, weighted_bipred_idc;
    int32_t pic_init_qp, pic_init_qs, chroma_qp_index_offset;
    int32_t deblocking_filter_control_present, constrained_intra_pred, redundant_pic_cnt_present;
    int32_t has_tail, transform_8x8_mode, pic_scaling_matrix_present, second_chroma_qp_index_offset;
} pcamv_pps_t;
int pcamv_gpu_parse_sps(const uint8_t *rbsp, size_t len, pcamv_sps_t *out);
int pcamv_gpu_parse_pps(const uint8_t *rbsp, size_t len, pcamv_pps_t *out);
/* The parameter sets of one stream, resolved: status, the picture size, and n_pps entries sorted by pps_id ascending, each a PPS merged
 * with the SPS it names into what the slice-header reader takes (log2_max_poc_lsb 4 where poc_type is not 0: it is not read then).
 *  1. The units considered are the stream's units of nal_unit_type 7 and 8, in stream order, as pcamv_gpu_annexb_index cuts them.  More
 *     than PCAMV_PSET_UNITS_MAX of them: PCAMV_EUNSUP for the stream, before anything else.  A unit longer than PCAMV_PSET_UNIT_BYTES has
 *     the code PCAMV_EUNSUP.
 *  2. Each other unit is unescaped as by pcamv_gpu_nal_to_rbsp, whose failure is the unit's code, and then parsed.
 *  3. The stream's status is the code of the first unit, in stream order, whose code is not 0 -- whether anything names that set or not.
 *  4. Else the units are walked in stream order: at most PCAMV_PSET_SPS_MAX distinct sps_id and PCAMV_PSET_PPS_MAX distinct pps_id, and a
 *     set sent again must equal the earlier one of its id member by member; the first unit that breaks either is PCAMV_EUNSUP.
 *     Position does not matter: parameter sets are constant over a stream in this path, and a PPS may precede its SPS.
 *  5. Else: no PPS at all is PCAMV_EINVAL; a PPS that names no SPS of the stream is PCAMV_EINVAL; SPS named by PPS that differ in mb_w x
 *     mb_h are PCAMV_EUNSUP -- judged in this order.
 * With a non-zero status mb_w, mb_h, n_pps and every entry are 0. */
#define PCAMV_PSET_UNITS_MAX 64
#define PCAMV_PSET_UNIT_BYTES 1024
#define PCAMV_PSET_SPS_MAX 4
#define PCAMV_PSET_PPS_MAX 8
typedef struct pcamv_param_sets_t {
    int32_t status, mb_w, mb_h, n_pps;
    pcamv_stream_params_t pps[PCAMV_PSET_PPS_MAX];
} pcamv_param_sets_t;
int pcamv_gpu_stream_param_sets(const uint8_t *bytes, size_t len, pcamv_param_sets_t *out);
/* pcamv_gpu_parse_slice_header under a stream's sets: with a non-zero status that status for every header; else exactly
 * pcamv_gpu_parse_slice_header under the entry whose pps_id is the header's, PCAMV_EUNSUP if there is none (failures found before pps_id
 * is read are the same under any parameters).  *entropy_cabac (optional): the entry's entropy mode, -1 where no entry was reached. */
int pcamv_gpu_parse_slice_header_sets(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_param_sets_t *sets, int64_t *start_bit,
                                      int32_t *slice_qp, int32_t *frame_num, int32_t *entropy_cabac);
/* The inverse, for the sender's `head`.  write_sps / write_pps write what the parsers read, with vui_parameters_present_flag 0 (the member
 * is not looked at), for poc_type 1 a cycle of num_ref_frames_in_poc_cycle offsets 0, no optional PPS tail (has_tail must be 0 and the
 * second chroma offset the first, else PCAMV_EINVAL), and rbsp_trailing_bits; they refuse, member by member in syntax order and with the
 * parsers' codes, what the parsers refuse.  rbsp[cap] receives *len bytes (at most PCAMV_PSET_RBSP_MAX); cap too small: PCAMV_ENOMEM.
 * param_set_head: an SPS unit (header byte 0x67) and a PPS unit (0x68) for `params` and a picture of mb_w x mb_h macroblocks, each with
 * a long start code and emulation prevention (pcamv_gpu_rbsp_to_nal): constraint byte 0, frame macroblocks, 4:2:0, 8 bits, no cropping,
 * direct_8x8_inference_flag 1, the POC type of `params` (type 1 with an empty cycle and offsets 0), one slice group, one default reference
 * in list 1, pic_init_qs 26, chroma offset 0 -- what pcamv_gpu_batch_stream_open takes as head, or as its start. */
#define PCAMV_PSET_RBSP_MAX 384
int pcamv_gpu_write_sps(const pcamv_sps_t *sps, uint8_t *rbsp, size_t cap, size_t *len);
int pcamv_gpu_write_pps(const pcamv_pps_t *pps, uint8_t *rbsp, size_t cap, size_t *len);
int pcamv_gpu_param_set_head(const pcamv_stream_params_t *params, int mb_w, int mb_h, int sps_id, int num_ref_frames, int profile_idc, int level_idc,
                             uint8_t *out, size_t cap, size_t *len);
/* stream_param_sets: behind an index call (before one: PCAMV_EINVAL).  The parameter-set units of every indexed stream are found by a
 * second run of the index kernels that selects types 7 and 8 (the index call itself costs what it did), unescaped one wavefront per
 * unit into slots of PCAMV_PSET_UNIT_BYTES (k_pset_unit), parsed one lane per unit (k_pset_parse) and resolved one wavefront per stream
 * (k_pset_resolve) by the rules above; a stream whose mb_w x mb_h is not the context's gets PCAMV_EUNSUP, one the index call refused
 * PCAMV_EINVAL.  The sets stay on the device until the next index call.  The call waits for the device three times: for the whole device
 * at its start (steps under the sets it replaces may be in flight on any stream), for `stream` in its middle -- the working memory is
 * sized by the counts the scan found, not by n x 64 x 1 KB, and the places of the units go up with small blocking copies -- and for
 * `stream` at its end, when it returns each context's status (host int32, optional) and the sets (host structs, optional).
 * extract_stream_step_sets / extract_stream_window_sets: pcamv_gpu_batch_extract_stream_step / _window without `params` -- each header
 * is read under its context's table (k_slice_header_sets).  PCAMV_EINVAL for the whole call if no stream_param_sets call followed the
 * last index call.  The parser is the one of the contexts' own entropy mode: a batch holds contexts of one mode (pcamv_gpu_batch_create
 * refuses others), so a batch of both modes cannot reach these calls.  Cursor,
 * PCAMV_EEOF and kind-UNSUP handling are those calls'.  A context whose sets have a non-zero status still takes its unit and its cursor
 * moves; it reports that status and appends nothing.  A slice whose PPS states the other entropy mode than its context's b_cabac is
 * PCAMV_EUNSUP, judged where pps_id is.  No host synchronisation and no per-frame host arrays.  For a batch whose streams all carry
 * the parameter sets P these calls are observationally the calls above with params = P.
 * param_sets_device: the parity probe; n streams of one host buffer through the same kernels (no picture size is compared), the sets to
 * sets_out[n].  Synchronises. */
int pcamv_gpu_batch_stream_param_sets(pcamv_batch_t *batch, int32_t *status_out, pcamv_param_sets_t *sets_out, void *stream);
int pcamv_gpu_batch_extract_stream_step_sets(pcamv_batch_t *batch, float emrate, int32_t *nal_header, void *stream);
int pcamv_gpu_batch_extract_stream_window_sets(pcamv_batch_t *batch, float emrate, int k, int32_t *nal_header, void *stream);
int pcamv_gpu_param_sets_device(pcamv_ctx_t *ctx, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                pcamv_param_sets_t *sets_out);

/* ---- One video of many chains: streams joined on the sender, the video cut at IDR units on the receiver (PCAMV_FEATURE_VIDEO) ----
 *
 * A chain is one closed GOP; a video is the chains' streams behind each other, each with an IDR picture of its own at its head.  The
 * calls above write and read one stream per context.  With these the sender gives every context its own head, appends the contexts'
 * streams to one video on the device, and the receiver is handed that video and nothing else: GOP g goes to context g - first_gop.  As
 * everywhere here the host function is the definition on every input, valid or not.
 *
 * annexb_gops, host code.  U[0 .. m) are the units of bytes[0, len) as pcamv_gpu_annexb_index lists them; the type of a unit is
 * nal_header & 31, an empty unit has none; VCL means types 1 .. 5.  Unit u opens a GOP iff its type is 5 and the nearest VCL unit
 * before it, if there is one, is not of type 5: the IDR slices of one picture, and IDR pictures directly behind each other, stay in one
 * GOP.  The GOP's first unit f is the unit behind that nearest VCL unit (0 if there is none), so delimiters, SEI and parameter sets in
 * front of the IDR unit belong to the GOP; its first byte is U[f - 1].off + U[f - 1].len (0 for f = 0), so the zeros and the start code
 * go with the unit they introduce.  GOP g is the bytes from its first byte to the next GOP's first byte, or to len; n_units likewise
 * counts to the next GOP's first unit, or to m.  *preamble: the bytes in front of the first GOP (units before any IDR picture, which
 * belong to no context), len if there is no GOP.  gops[cap] receives the first cap GOPs, *n_gops counts them all. */
typedef struct pcamv_gop_t { int64_t off, len, first_unit, n_units; } pcamv_gop_t;
int pcamv_gpu_annexb_gops(const uint8_t *bytes, size_t len, pcamv_gop_t *gops, size_t cap, int64_t *n_gops, int64_t *preamble);
/* stream_open_heads: pcamv_gpu_batch_stream_open with a head per context.  `heads` is a borrowed device buffer of heads_size bytes (at
 * most 2^40) that the queued work reads; head_off / head_len are device int64 arrays of one entry per context, read by this call alone
 * like off / cap.  Observationally the call is stream_open with head = heads[head_off[i] .. + head_len[i]) for context i, its refusal
 * rules and len[i] included; a context whose head does not lie inside `heads`, is longer than 2^24 or does not fit its region gets len 0
 * and PCAMV_EINVAL in every step, and nothing is written for it.  The decision is made on the device, one lane per context
 * (k_stream_open_heads); the bytes go through k_stream_copy: one wavefront per PCAMV_STREAM_CHUNK destination bytes of a head, whole
 * aligned dwords (16 bytes per lane where all of them are the head's) and single bytes at the two ends only.  The call waits once for
 * `stream`, as stream_open does, and for none of its kernels.
 *
 * join_streams: behind an open of either kind (before one: PCAMV_EINVAL).  video_off (device int64[1]) and video_len (device int64[1],
 * in and out) say where in `video` (a borrowed device buffer of video_size bytes) the video begins and how long it is so far; the
 * streams of contexts 0 .. n - 1, as long as they are on `stream` at that point, are appended in context order and video_len grows by
 * their sum.  placed (device int64[n], optional) receives where each context's bytes went, counted from video_off, -1 for a context whose
 * stream is empty or whose open was refused.  Such a context contributes nothing, so THE GOPS BEHIND IT MOVE UP BY ONE in the video:
 * `placed` is how the caller learns of it.  If video_off or video_len is negative or the sum does not fit video_size, nothing is written,
 * video_len stays, every placed[i] is -1 and the status is PCAMV_ENOMEM.  pcamv_gpu_batch_join_status synchronises and returns the last
 * join's status as its value.  `video` overlapping the open buffer, or an open buffer of more than 2^40 bytes: PCAMV_EINVAL, judged on
 * the host before anything is queued.  The call does not synchronise: it queues k_stream_join (one wavefront: a lane-parallel prefix over
 * the lengths), k_stream_copy_plan and k_stream_copy.  Appending is what lets a video of more GOPs than contexts be written in rounds.
 *
 * index_video_device: off / len are device int64[1] -- what a join left can be handed over as it is -- and describe one video inside
 * `bytes` (borrowed until the next index call).  Observationally: pcamv_gpu_annexb_gops on the video, then
 * pcamv_gpu_batch_index_streams_device with context i's stream set to GOP first_gop + i; a context past the last GOP gets the length 0,
 * so its count is 0 and every step is PCAMV_EEOF.  *n_gops / *preamble (host, optional) are the video's, whatever first_gop is.  A video
 * that does not lie inside `bytes`: PCAMV_EINVAL.  On the device the index kernels list ALL units of the video into a table sized by the
 * counts their first scan found (the prefix over the one long stream's chunks runs in two levels on many wavefronts, k_video_prefix_*;
 * k_stream_prefix walks a stream's chunks with one); k_video_cut, one wavefront, walks it in passes of 64 units and writes every context's (off, len), which
 * the index kernels then take as they take a caller's.  TWO host synchronisations: one for the unit count that sizes the table, one at
 * the end as in every index call.  One video per call.  index_video is the same on host bytes, staged with one copy.
 * Behind an index_video call stream_param_sets resolves the parameter sets of the VIDEO once, by the rules above (units of type 7 / 8
 * anywhere in it, position not mattering), and every context reads its slice headers under that one table; status_out / sets_out return
 * it per context.  GOPs behind the first often carry no parameter sets of their own.  Behind a plain index call nothing changes; an index
 * call of either kind decides which holds.
 * video_gops_device: the parity probe; n videos of one host buffer through the same kernels, gops_out n tables of cap_per_video +
 * PCAMV_UNIT_GUARD entries each (every byte 0xA5 beforehand; the first min(n_gops, cap_per_video) are filled), n_gops[i] / preamble[i]
 * as annexb_gops gives them (both PCAMV_EINVAL for a video outside the buffer).  Synchronises. */
int pcamv_gpu_batch_stream_open_heads(pcamv_batch_t *batch, void *bytes, size_t bytes_size, const int64_t *off, const int64_t *cap, int64_t *len,
                                      const pcamv_stream_params_t *params, const pcamv_stream_write_t *wr, const void *heads, size_t heads_size,
                                      const int64_t *head_off, const int64_t *head_len, void *stream);
int pcamv_gpu_batch_join_streams(pcamv_batch_t *batch, void *video, size_t video_size, const int64_t *video_off, int64_t *video_len, int64_t *placed,
                                 void *stream);
int pcamv_gpu_batch_join_status(pcamv_batch_t *batch);
int pcamv_gpu_batch_index_video_device(pcamv_batch_t *batch, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                       int64_t first_gop, int64_t max_units, int64_t *n_gops, int64_t *preamble, int64_t *n_slices_out, void *stream);
int pcamv_gpu_batch_index_video(pcamv_batch_t *batch, const uint8_t *bytes, size_t len, int64_t first_gop, int64_t max_units, int64_t *n_gops,
                                int64_t *preamble, int64_t *n_slices_out, void *stream);
int pcamv_gpu_video_gops_device(pcamv_ctx_t *ctx, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                pcamv_gop_t *gops_out, int64_t cap_per_video, int64_t *n_gops, int64_t *preamble);

/* ---- IDR pictures coded on the device: the picture every chain starts with (PCAMV_FEATURE_IDR) ----
 *
 * The calls above predict a chain's first P picture from a reference the caller brought.  With these the library makes that picture
 * itself: a context's source coded as one IDR I slice on the device, its reconstruction installed as the context's reference, its unit
 * put into the context's stream.  Scope, fixed: one slice per picture (or, with the *3 calls below, several of whole rows), Intra16x16 macroblocks only -- luma vertical / horizontal / DC /
 * plane and the four chroma modes, chosen per macroblock by SATD among the modes whose neighbours exist -- one QP (mb_qp_delta 0), the
 * intra dead zone i_luma_deadzone[1] and the context's i_chroma_qp_offset, CAVLC slice data whatever the context's b_cabac (an IDR slice
 * names a PPS of its own: a CABAC stream carries a second PPS with entropy_coding_mode_flag 0, which is legal), no loop filter
 * (disable_deblocking_filter_idc 1, so that PPS needs deblocking control).  Every quantised level is clamped to +-2063, the largest
 * magnitude level_prefix 15 expresses at every suffix length, before the reconstruction (csrc/pcamv_idr.h derives it).  NOT the
 * reference's I-frame coder, and not bit-equal with it: an I picture carries no payload, and exact here means that a decoder
 * reconstructs precisely the planes the chain predicts from.
 *
 * write_idr_slice_header / parse_idr_slice_header: host code, no GPU; the definition on every input.  slice_header() (7.3.3) of an IDR I
 * slice: first_mb_in_slice 0, slice_type 7, pps_id, frame_num 0, idr_pic_id, the POC elements of the POC type (all zero),
 * redundant_pic_cnt 0 if present, no_output_of_prior_pics_flag 0, long_term_reference_flag 0, slice_qp_delta,
 * disable_deblocking_filter_idc 1.  The writer refuses before anything is written: PCAMV_EINVAL for params outside their ranges,
 * nal_ref_idc outside 1 .. 3, idr_pic_id outside 0 .. 65535, slice_qp outside 0 .. 51; then PCAMV_EUNSUP for weighted_pred, entropy_cabac
 * and a PPS without deblocking control; PCAMV_ENOMEM for cap too small.  bits / n_bits as pcamv_gpu_write_slice_header gives them.
 * The parser reads rbsp[0, len) (the unit behind its header byte, unescaped) under the rules of pcamv_gpu_parse_slice_header -- a read
 * failure is PCAMV_EINVAL and found before the element is judged: nal_unit_type != 5, first_mb_in_slice != 0, slice_type not 2 or 7, another
 * pps_id: PCAMV_EUNSUP; frame_num != 0 or idr_pic_id above 65535: PCAMV_EINVAL; long_term_reference_flag 1, entropy_cabac, no deblocking
 * control or an idc of 0 or 2: PCAMV_EUNSUP; a QP outside 0 .. 51 or an idc above 2: PCAMV_EINVAL.  All three outputs are -1 on failure.
 *
 * decode_islice_cavlc: host code, no GPU.  An independent decoder of exactly this subset -- Intra16x16, CAVLC, one QP, no filter -- from
 * bit start_bit of the RBSP; y / u / v receive the planes tightly packed (16 mb_w x 16 mb_h, half that twice).  PCAMV_EUNSUP for any other
 * macroblock type or a non-zero mb_qp_delta, PCAMV_EINVAL for bad data (a read past the end, a code no table holds, a level_prefix above
 * 15, a mode whose neighbours are missing, coefficients past a block's end, anything but rbsp_trailing_bits behind the last macroblock).
 * With the device coder it shares the code tables and nothing else: it is what the tests hold the device to, and what a user calls to see
 * the picture.
 *
 * encode_idr: the probe; synchronises.  The context's current source at `qp` as one IDR slice: out[cap] receives *len bytes, the RBSP or
 * (as_nal) the unit with long start code, header byte 0x65 and emulation prevention; the header is write_idr_slice_header's for
 * pcamv_stream_params_t {4, 0, 4, 0, 0, 0, 1, 0, 0, 26, 1, pps_id} and nal_ref_idc 3.  The unfiltered reconstruction is installed as the
 * context's reference, as a host set_ref with no previous motion installs one (the rule under "what a context remembers"), and is
 * readable through fetch_recon / recon_device / get_ref_planes.  A unit that does not fit is PCAMV_ENOMEM; the reference is installed all
 * the same.  idr_bound: a capacity that always fits.
 *
 * write_stream_idr: behind stream_open / stream_open_heads and before the first write_stream_step since that open, else PCAMV_EINVAL; the
 * open must have first_pic 0, else PCAMV_EINVAL; the stream's PPS must have deblocking control, else PCAMV_EUNSUP; all before anything is
 * queued.  Every context's source becomes picture 0 of its stream, [09 10 delimiter +] IDR unit of the stream's nal_ref_idc behind the
 * head (which now holds parameter sets only), under the stream's parameter sets with pps_id as given and entropy_cabac 0; every context
 * gets its reference; the picture counter moves to 1, so the first P picture has frame_num 1 and poc_lsb 2 by the rule of
 * pcamv_stream_write_t.  No host synchronisation.  pcamv_gpu_batch_write_status reports 0 / PCAMV_ENOMEM (stream and len[i] unchanged) /
 * PCAMV_EINVAL as for a step; a picture that did not fit still installs the reference and moves the counter, as a P picture does.
 * Kernels (pcamv_gpu_batch_kernel_time knows them by name): k_idr_mb, one wavefront per macroblock, one launch per anti-diagonal x + y;
 * k_idr_prefix; k_idr_pack, one lane per dword of the RBSP; k_idr_unit, one wavefront per context; k_stream_commit.  The working memory
 * is the batch's, made at first use and released with it: 2842 bytes per macroblock and place, at most 8 GiB; larger batches run their
 * contexts in groups inside the call.
 *
 * Filtered IDR pictures (PCAMV_FEATURE_IDR_DEBLOCK): the calls that end in 2 take `deblock`, 0 or 1 (anything else PCAMV_EINVAL, judged
 * with the other values); with 0 each is its namesake byte for byte, refusals included.  With 1 the picture goes through the loop
 * filter of 8.7 before it becomes the reference -- as every P picture behind it does -- and its header says so:
 * disable_deblocking_filter_idc 0 with both offsets 0 under a PPS with deblocking control (the header is as long as the unfiltered
 * one's), no deblocking element at all under a PPS without it, where the filter is on by inference (3 bits shorter); so a PPS without
 * deblocking control is no longer refused, by the header writer and by write_stream_idr2.  The slice data is the same bits either way:
 * intra prediction reads unfiltered samples, so the filter runs behind the whole picture's coding.
 * deblock_intra_picture: host code, no GPU; the definition of the filter on every input.  8.7 for a frame picture of one slice, Intra16x16
 * macroblocks only, one QP, 4x4 transform, FilterOffsetA = FilterOffsetB = 0, in place on tightly packed planes, macroblock by
 * macroblock in raster order: bS 4 on a macroblock edge whose neighbour lies in the picture, 3 on the inner edges, the picture's border
 * not filtered; indexA = indexB = qp for luma, the chroma QP of qp + chroma_qp_index_offset for both chroma planes.  PCAMV_EINVAL for a
 * NULL plane, a size outside decode_islice_cavlc's, a QP outside 0 .. 51, an offset outside -12 .. 12.
 * parse_idr_slice_header2: as parse_idr_slice_header up to slice_qp_delta; then *disable_deblocking_filter_idc receives 0, 1 or 2 (one
 * slice per picture: 2 filters as 0 does), 0 under a PPS without deblocking control; an offset that is not 0 is PCAMV_EUNSUP, one outside
 * -6 .. 6 and an idc above 2 PCAMV_EINVAL.  All four outputs are -1 on failure.  A decoder of these pictures is decode_islice_cavlc
 * followed, unless the idc is 1, by deblock_intra_picture.
 * Kernel: k_idr_deblock (csrc/pcamv_idr_deblock.h), one wavefront per macroblock, one launch per anti-diagonal x + 2 y over all contexts
 * of the call, behind the coder's groups and before the pictures become the references.
 *
 * Several slices per picture (PCAMV_FEATURE_IDR_SLICES): the calls that end in 3 take `slice_rows` R, the macroblock rows of a slice.  R = 0
 * or R >= mb_h: one slice, the *2 call byte for byte through the same launches.  1 <= R < mb_h: S = ceil(mb_h / R) slices, slice s the rows
 * [s R, min((s + 1) R, mb_h)), the last one possibly shorter.  R < 0 is PCAMV_EINVAL, judged with the other values before anything is
 * queued.  Slices are whole rows: a macroblock's left neighbour is always in its slice, its top and top-left neighbours are there
 * together or not at all.  A macroblock is coded as before with "available" meaning "in the slice": the modes to choose among, the
 * prediction, nC of 9.2.1.  Every slice's header says the same -- slice_type 7, pps_id, frame_num 0, idr_pic_id, the POC elements,
 * slice_qp_delta, the deblocking elements -- but for first_mb_in_slice = s R mb_w; one access unit delimiter per picture, in front of
 * slice 0.  deblock 1: idc 0, the filter crosses slice edges and is the one-slice picture's (bS 4 / 3 by position); deblock 0: idc 1 in
 * every slice.  P pictures stay one slice per picture.
 * write_idr_slice_header3: header2 with first_mb_in_slice = first_mb, 0 .. 2^20 - 1 (else PCAMV_EINVAL, with the other values).
 * parse_idr_slice_header3: header2's parser that reads first_mb_in_slice into *first_mb (above 2^20 - 1: PCAMV_EINVAL) where the others
 * refuse a value that is not 0; all five outputs -1 on failure.
 * encode_idr3: with S > 1, out receives the S units behind each other and as_nal must be 1 (RBSPs behind each other mean nothing):
 * PCAMV_EINVAL otherwise, before anything is queued.  A capacity below the sum of the units is PCAMV_ENOMEM.  idr_bound3: the sum of
 * idr_bound over the slices.
 * write_stream_idr3: the stream receives [delimiter +] the S units back to back; they fit together or the stream and len[i] stay as they
 * are (PCAMV_ENOMEM), as a delimiter and its unit do.  The picture counter moves by 1, the unit counter (stream_written's third value) by S.
 * The receiving side needs nothing: the IDR slices of one picture stay in one GOP (the rule at "One video of many chains") and are
 * PCAMV_UNIT_OTHER in an index.
 * decode_idr_picture: host code, no GPU; the definition the device is held to.  bytes[0, len) is Annex B; its units of type 5 are the
 * picture's slices in order, units that are no VCL units are passed over.  Every header is read by parse_idr_slice_header3 under params;
 * each slice is decoded by decode_islice_cavlc as a picture of its own rows into the planes y / u / v (16 mb_w x 16 mb_h, half that
 * twice), and unless the idc is 1 the whole picture then goes through deblock_intra_picture.  PCAMV_EUNSUP: a first_mb that is no
 * multiple of mb_w; slices out of order, overlapping or not covering the picture (a slice that does not end where the next begins, or
 * the last one at the picture's end, fails its decoder's end-of-slice rule and is reported so); slices that disagree in QP, idr_pic_id
 * or idc; idc 2 with more than one slice; a VCL unit of another type among them.  No slice at all: PCAMV_EINVAL.  *n_slices: how many.
 * Kernels with S > 1: k_idr_mb as before; k_idr_prefix restarts at every slice behind that slice's header; k_idr_pack works per (slice,
 * context); k_idr_unit_len, one wavefront per (context, slice), counts the unit's bytes by the writer's own walk with the stores
 * suppressed; k_idr_place, one lane per context, places the units or refuses them all; k_idr_unit, one wavefront per (context, slice),
 * writes at its place -- units that are neighbours share a dword, and no dword store covers a byte outside the unit's own.  With S = 1
 * there is no length pass.  Working memory: 2842 bytes per macroblock and place as before, and 64 S per place (a prefix entry, a header's
 * room in the RBSP, a unit's length and offset); the 8 GiB cap and the groups stand.
 *
 * Intra4x4 macroblocks (PCAMV_FEATURE_IDR_I4X4): the calls that end in 4 take `i4x4` -- 0: every macroblock Intra16x16, and the call IS its
 * *3 sibling, byte for byte and launch for launch; 1: per macroblock Intra4x4 where it costs less; 2: every macroblock Intra4x4 (a probe
 * setting, and the smallest pictures on noisy content); anything else PCAMV_EINVAL before anything is queued.  The rule (the coder's own,
 * not the reference's; csrc/pcamv_idr_i4x4.h): the macroblock is coded as before, which gives cost16, the SATD of the winning Intra16x16
 * mode; then the sixteen 4x4 blocks in luma4x4BlkIdx order, each with the modes of 8.3.1.2 whose neighbours exist in the slice, cost
 * SATD + lambda (1 for the predicted mode of 8.3.1.1, 4 for another), lambda the analysis' own at this QP, the lowest cost winning and
 * ties going to the lower mode; every block transformed, quantised with the intra dead zone and the clamp of the other levels, and
 * reconstructed before the next is predicted.  Intra4x4 iff 24 lambda + the sixteen costs < cost16.  Chroma is coded as before in
 * both types.  An Intra4x4 macroblock is at most 11230 bits, 51 more than an Intra16x16 one, so idr_bound4 with i4x4 != 0 is larger
 * than idr_bound3; the slot of a macroblock stays, the RBSP of a place grows by 6.4 bytes a macroblock and a place holds 16 more (the
 * modes the neighbours read) in such calls only.  Kernel: k_idr_mb4 in k_idr_mb's place, one wavefront per macroblock, one launch per
 * anti-diagonal x + 2 y (Intra4x4 reads the macroblock above-right); every other kernel is the same.  The loop filter is the same:
 * with the 4x4 transform bS is 4 on macroblock edges and 3 inside for every intra macroblock.
 * decode_islice_cavlc2 / decode_idr_picture2: `flags` bit 0 makes the host decoder accept I_NxN macroblocks (its own nine predictors,
 * the intra column of Table 9-4, mb_qp_delta only with a pattern, nC across the macroblock types); other bits PCAMV_EINVAL; with flags 0
 * they are the functions without the 2, which go on refusing mb_type 0 with PCAMV_EUNSUP.  With the flag: a mode whose neighbours do
 * not exist and a pattern codeNum above 47 are PCAMV_EINVAL, mb_qp_delta != 0 PCAMV_EUNSUP. */
int pcamv_gpu_encode_idr4(pcamv_ctx_t *ctx, int qp, int pps_id, int idr_pic_id, int as_nal, int deblock, int slice_rows, int i4x4, uint8_t *out, size_t cap, size_t *len);
int pcamv_gpu_batch_write_stream_idr4(pcamv_batch_t *batch, int qp, int pps_id, int idr_pic_id, int deblock, int slice_rows, int i4x4, void *stream);
int64_t pcamv_gpu_idr_bound4(const pcamv_ctx_t *ctx, int as_nal, int slice_rows, int i4x4);
int pcamv_gpu_decode_islice_cavlc2(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, int slice_qp, int chroma_qp_index_offset, int flags,
                                   uint8_t *y, uint8_t *u, uint8_t *v);
int pcamv_gpu_decode_idr_picture2(const uint8_t *bytes, size_t len, int mb_w, int mb_h, const pcamv_stream_params_t *params, int chroma_qp_index_offset, int flags,
                                  uint8_t *y, uint8_t *u, uint8_t *v, int32_t *slice_qp, int32_t *idr_pic_id, int32_t *n_slices);
int pcamv_gpu_write_idr_slice_header3(const pcamv_stream_params_t *params, int nal_ref_idc, int idr_pic_id, int slice_qp, int deblock, int64_t first_mb, uint8_t *bits,
                                      size_t cap, int32_t *n_bits);
int pcamv_gpu_parse_idr_slice_header3(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                      int32_t *slice_qp, int32_t *idr_pic_id, int32_t *disable_deblocking_filter_idc, int64_t *first_mb);
int pcamv_gpu_encode_idr3(pcamv_ctx_t *ctx, int qp, int pps_id, int idr_pic_id, int as_nal, int deblock, int slice_rows, uint8_t *out, size_t cap, size_t *len);
int pcamv_gpu_batch_write_stream_idr3(pcamv_batch_t *batch, int qp, int pps_id, int idr_pic_id, int deblock, int slice_rows, void *stream);
int64_t pcamv_gpu_idr_bound3(const pcamv_ctx_t *ctx, int as_nal, int slice_rows);
int pcamv_gpu_decode_idr_picture(const uint8_t *bytes, size_t len, int mb_w, int mb_h, const pcamv_stream_params_t *params, int chroma_qp_index_offset,
                                 uint8_t *y, uint8_t *u, uint8_t *v, int32_t *slice_qp, int32_t *idr_pic_id, int32_t *n_slices);
int pcamv_gpu_write_idr_slice_header2(const pcamv_stream_params_t *params, int nal_ref_idc, int idr_pic_id, int slice_qp, int deblock, uint8_t *bits, size_t cap,
                                      int32_t *n_bits);
int pcamv_gpu_parse_idr_slice_header2(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                      int32_t *slice_qp, int32_t *idr_pic_id, int32_t *disable_deblocking_filter_idc);
int pcamv_gpu_deblock_intra_picture(uint8_t *y, uint8_t *u, uint8_t *v, int mb_w, int mb_h, int qp, int chroma_qp_index_offset);
int pcamv_gpu_encode_idr2(pcamv_ctx_t *ctx, int qp, int pps_id, int idr_pic_id, int as_nal, int deblock, uint8_t *out, size_t cap, size_t *len);
int pcamv_gpu_batch_write_stream_idr2(pcamv_batch_t *batch, int qp, int pps_id, int idr_pic_id, int deblock, void *stream);
int pcamv_gpu_write_idr_slice_header(const pcamv_stream_params_t *params, int nal_ref_idc, int idr_pic_id, int slice_qp, uint8_t *bits, size_t cap, int32_t *n_bits);
int pcamv_gpu_parse_idr_slice_header(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                     int32_t *slice_qp, int32_t *idr_pic_id);
int pcamv_gpu_decode_islice_cavlc(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, int slice_qp, int chroma_qp_index_offset,
                                  uint8_t *y, uint8_t *u, uint8_t *v);
int pcamv_gpu_encode_idr(pcamv_ctx_t *ctx, int qp, int pps_id, int idr_pic_id, int as_nal, uint8_t *out, size_t cap, size_t *len);
int64_t pcamv_gpu_idr_bound(const pcamv_ctx_t *ctx, int as_nal);
int pcamv_gpu_batch_write_stream_idr(pcamv_batch_t *batch, int qp, int pps_id, int idr_pic_id, void *stream);

/* ---- A QP per context, and rate control on the device (PCAMV_FEATURE_RATE) ----
 * pcamv_gpu_batch_step_qps: pcamv_gpu_batch_step with context i at qp[i] (a host array of the batch's size).  Any QP outside 0 .. 51
 * refuses the call (PCAMV_EINVAL) before anything is queued or any context has changed.  Nothing a batch chooses at its creation
 * depends on a QP: the build of the RD instance, the speculative chain, the flow queues and the trellis states per thread follow the
 * batch's size, the picture's width, the partitions and the search method alone, so contexts at different QPs share them.
 *
 * pcamv_gpu_batch_step_qp_device: the same with the QPs in device memory -- d_qp, int32 per context, borrowed for this call, read on
 * `stream` by the first kernel the call queues and by nothing later; no host synchronisation.  A value outside 0 .. 51 is clamped
 * before it indexes anything, and the context's status word says so (pcamv_gpu_batch_qp_status: 0 / PCAMV_EINVAL, of the last such
 * step).  How it works: the batch keeps, made by its first such call and equal to the host path by construction, one table of 52 rows
 * per distinct (i_chroma_qp_offset, i_luma_deadzone[0], i_luma_deadzone[1]) among its contexts (at most PCAMV_QP_TABLES_MAX, else
 * PCAMV_EUNSUP) -- a row is exactly what a host step at that QP writes into the frame descriptor: qp, chroma_qp, lambda, lambda2,
 * lambda2_chroma, the quantiser sets, and the pointers to the MV cost table and the slice-start context states -- and one copy of
 * those two tables that its contexts share, held only for the QPs allowed: all 52 (3.4 MB) for a caller's array, qp_min .. qp_max for a
 * rate (a later call that allows more makes them again for the union, behind a synchronisation).  k_frame_qp, queued behind the descriptor upload, copies each
 * context's row into its pushed descriptor, a dword per lane; every later kernel sees the descriptor a host step would have pushed.
 * The QP in force belongs to the CONTEXT: one device cell, written by the step.  While it is in force every descriptor push for the
 * context -- by any batch it is a member of, its own one-context batch included: write_stream_step, write_step*, write_pslice*,
 * pass2_pframe, extract_step -- is followed by the patch, so the calls behind such a step work at the step's QP.  It ends with the
 * context's next step or analysis at a host QP, or when the batch whose tables it uses is destroyed (the context then stands at the
 * QP of its last host step).  Probes that take a QP of their own (block_costs, rd_probe, encode_idr) keep theirs.
 * pcamv_gpu_qp_device / pcamv_gpu_batch_qps read the cells back (synchronising): the QP in force, or -1 where none is.
 *
 * The controller.  pcamv_gpu_batch_rate_open on a batch with open byte streams (else PCAMV_EINVAL; bad parameters PCAMV_EINVAL with
 * nothing opened; PCAMV_EUNSUP as above) gives every context a state on the device: qp = qp_init, debt = 0, last_len = the stream's
 * length as it stands on `stream`, pictures = 0.  While the rate is open, pcamv_gpu_batch_write_stream_step and
 * pcamv_gpu_batch_write_stream_idr* queue k_rate_update behind their k_stream_commit, and pcamv_gpu_batch_step_rate is
 * pcamv_gpu_batch_step_qp_device on the controller's own cells (PCAMV_EINVAL without a rate): a sender's loop is step_rate;
 * write_stream_step and nothing else.  An IDR picture's bytes count like any other's; its own QP stays the caller's argument.
 * pcamv_gpu_batch_stream_open* under an open rate is refused (PCAMV_EINVAL): close the rate first.  A message and a rate do not know of
 * each other.  pcamv_gpu_batch_rate_tell synchronises and copies the states out.
 * The rule, in integers only so that host and device agree bit for bit (pcamv_gpu_rate_update is its definition, without a GPU;
 * pcamv_gpu_rate_update_device runs n cases -- parameters, state, len and status of each -- through the kernel's code, one lane each).  With T = target_bits, W = window, len the
 * stream's length in bytes behind the picture:
 *   1. bits = 8 * clamp(len - last_len, 0, 2^41), then last_len = len;
 *   2. a write status that is not 0 (the picture did not fit): d = +max_step, debt unchanged;
 *   3. else debt = clamp(debt + bits - T, -2^40, 2^40);
 *   4. want = max(T - debt / W, T / 4, 1), divisions as C makes them;
 *   5. with P[0 .. 6] = {65536, 73562, 82570, 92682, 104032, 116772, 131072} (2^(k/6) in Q16): if bits >= want, d is the largest
 *      k <= max_step with bits * 65536 >= want * P[k]; else d is minus the largest k <= max_step with want * 65536 >= bits * P[k]
 *      (bits = 0: -max_step);
 *   6. qp = clamp(qp + d, qp_min, qp_max), pictures += 1.
 * Parameters: 1 <= target_bits <= 2^40, 0 <= qp_min <= qp_init <= qp_max <= 51, max_step 1 .. 6, window 1 .. 1024.
 * This is the library's own controller, not x264's ratecontrol.c (float arithmetic over complexity estimates the chain does not have);
 * nothing is claimed on how well it holds a bitrate on real content -- only the rule, and that device and host agree on it.
 * Out of scope: a QP per macroblock (mb_qp_delta), VBV, and the IDR picture's QP. */
#define PCAMV_QP_TABLES_MAX 8
typedef struct pcamv_rate_params_t { int64_t target_bits; int32_t qp_init, qp_min, qp_max, max_step, window, reserved; } pcamv_rate_params_t;
typedef struct pcamv_rate_state_t { int64_t debt, last_len, pictures; int32_t qp, last_d; } pcamv_rate_state_t;
int pcamv_gpu_batch_step_qps(pcamv_batch_t *batch, const int32_t *qp, float emrate, void *stream);
int pcamv_gpu_batch_step_qp_device(pcamv_batch_t *batch, const int32_t *d_qp, float emrate, void *stream);
int pcamv_gpu_batch_qp_status(pcamv_batch_t *batch, int32_t *status);
int pcamv_gpu_batch_qps(pcamv_batch_t *batch, int32_t *qp);
int pcamv_gpu_qp_device(pcamv_ctx_t *ctx, int32_t *qp);
int pcamv_gpu_batch_rate_open(pcamv_batch_t *batch, const pcamv_rate_params_t *params, void *stream);
int pcamv_gpu_batch_rate_close(pcamv_batch_t *batch);
int pcamv_gpu_batch_step_rate(pcamv_batch_t *batch, float emrate, void *stream);
int pcamv_gpu_batch_rate_tell(pcamv_batch_t *batch, pcamv_rate_state_t *states);
/* one picture through the rule: *state moves on, *d (optional) is the step.  PCAMV_EINVAL for parameters out of range (nothing changes) */
int pcamv_gpu_rate_update(const pcamv_rate_params_t *params, pcamv_rate_state_t *state, int64_t len, int32_t write_status, int32_t *d);
int pcamv_gpu_rate_update_device(pcamv_ctx_t *ctx, const pcamv_rate_params_t *params, pcamv_rate_state_t *states, const int64_t *len, const int32_t *write_status,
                                 int n, int32_t *d);

/* ---- The sender takes a video: pictures of any size, fed to all contexts on the device (PCAMV_FEATURE_SOURCE) ----
 * A context codes pictures of whole macroblocks (pcamv_gpu_open: width and height multiples of 16).  A source picture is width x height
 * luma samples, both even, with 16 (mb_w - 1) < width <= 16 mb_w and the same for the height, in 4:2:0: three planes (I420; YV12 with
 * planes 1 and 2 swapped, frame.c:206) or a luma plane and one plane of chroma pairs (NV12: U in the even bytes, V in the odd ones;
 * NV21 the other way round), lines top-down or bottom-up (PCAMV_SRC_VFLIP, as X264_CSP_VFLIP, frame.c:211-215).  A clip is a byte
 * range that holds pictures picture_stride bytes apart; plane k of a picture starts plane_off[k] bytes behind the picture's start and
 * its lines lie pitch[k] bytes apart (NV12 / NV21: two planes, the third entry is not looked at).  Nothing is asked of the alignment of
 * pitches, offsets or the clip's base.
 * The rule (x264_frame_copy_picture, then x264_frame_expand_border_mod16, common/frame.c:190-220 and 310-337): coded plane i, of
 * (16 mb_w >> !!i) x (16 mb_h >> !!i) samples, tightly packed, is
 *     out_i[y][x] = src_i[min(y, h_i - 1)][min(x, w_i - 1)],   w_i = width >> !!i, h_i = height >> !!i
 * -- the last real sample of a line repeated to the right, the last real line repeated downwards; with VFLIP src_i's line y is the
 * caller's line h_i - 1 - y.
 * pcamv_gpu_source_check validates a descriptor against a size in macroblocks and gives the number of whole pictures a clip of
 * clip_bytes holds: every byte a picture index below that number reads lies inside the clip, and no byte is read that the rule does
 * not name (bytes between a line's end and the next line, or between planes, may be unmapped).  PCAMV_EINVAL: an odd size, a size
 * outside the macroblock grid, a pitch below a line's bytes (width for luma and for a plane of pairs, width / 2 for a planar chroma
 * plane), an unknown format or flag, a negative offset, picture_stride < 1, or an offset, pitch or picture_stride above 2^40.
 * pcamv_gpu_source_picture is the definition, sequential and naive: picture `picture` of a host clip into out[3] (PCAMV_EINVAL also
 * for an index outside 0 .. n_pictures - 1).  pcamv_gpu_upload_picture runs it into a staging buffer and then does what
 * pcamv_gpu_upload_fenc does: a host caller gets the same rule, and it is the parity probe beside the kernel.
 *
 * pcamv_gpu_batch_feed_device: one launch of k_source_feed over all contexts of the batch, queued on `stream` (NULL: the first
 * context's), no host synchronisation: context i gets picture d_picture[i] (device int64, one per context) of the clip at d_clip
 * (device memory, clip_bytes long), padded, into its own source planes -- the ones pcamv_gpu_upload_fenc fills -- and stands as
 * pcamv_gpu_upload_fenc leaves a context: the planes are its source (a pcamv_gpu_set_fenc_device before is undone, one after takes over
 * again), and a second pass re-encodes every macroblock.  Clip and indices are borrowed until the queued work has run; the caller moves
 * the indices on with a device add, and a sender's loop is feed; step_rate; write_stream_step.  Ordering is the caller's: whatever
 * writes d_picture or the clip must be ordered against `stream` -- queue the add on the stream handed to this call, and the calls that
 * read the source (the step, write_stream_idr) on it too; with stream == NULL the feed runs on the first context's own stream, which is
 * non-blocking (the null stream orders nothing against it) and which the caller cannot name: synchronise before the call then.  An index outside 0 .. n_pictures - 1
 * gives that context the status PCAMV_EINVAL (pcamv_gpu_batch_feed_status, which synchronises; 0 otherwise, and 0 before any feed) and
 * nothing of its planes is written; the others are unaffected.  A descriptor pcamv_gpu_source_check refuses for the contexts' size
 * refuses the call with nothing queued.  The batch's first feed makes, once for good, the table of its contexts' plane addresses and
 * the status words.
 * The kernel: a wavefront per (context, macroblock row of luma | macroblock row of both chroma planes); the destination bytes of such
 * a work item are one contiguous span of a tight plane, stored 16 bytes a lane (8 in chroma rows of an odd mb_w, which are only 8-byte
 * aligned), 64 lanes side by side; loads are as wide as the source address allows at run time (the source tells 16, 8, 4, 2 and 1
 * bytes apart; in the gfx950 code object the 4- and 2-byte cases are unaligned 8- and 16-byte loads, which the hardware serves); a
 * chunk that crosses the picture's right edge is read byte by byte.
 *
 * pcamv_gpu_param_set_head2: pcamv_gpu_param_set_head for a picture of width x height samples, both even (else PCAMV_EINVAL):
 * mb_w = (width + 15) / 16, mb_h likewise; frame_cropping_flag 1 iff a size is no multiple of 16, with frame_crop_right_offset
 * (16 mb_w - width) / 2, frame_crop_bottom_offset (16 mb_h - height) / 2, left and top 0 (encoder/set.c:139-143, 275-281).  For sizes
 * that are multiples of 16 the bytes are pcamv_gpu_param_set_head's.  A receiver reads the size back from the SPS (pcamv_gpu_parse_sps:
 * 16 mb_w - 2 (crop_left + crop_right) by 16 mb_h - 2 (crop_top + crop_bottom)); pcamv_param_sets_t and the device-side receiver need
 * the size in macroblocks only and stay as they are.
 * Out of scope: RGB, 4:2:2 and 4:4:4 input (the reference refuses them too, frame.c:194), interlaced pictures. */
#define PCAMV_SRC_I420 0
#define PCAMV_SRC_YV12 1
#define PCAMV_SRC_NV12 2
#define PCAMV_SRC_NV21 3
#define PCAMV_SRC_VFLIP 1
typedef struct pcamv_source_t {
    int32_t width, height;     /* the picture's own luma size: even, 16 (mb_w - 1) < width <= 16 mb_w, the same for height */
    int32_t format;            /* PCAMV_SRC_I420 | PCAMV_SRC_YV12 | PCAMV_SRC_NV12 | PCAMV_SRC_NV21 */
    int32_t flags;             /* PCAMV_SRC_VFLIP: lines bottom-up */
    int64_t plane_off[3];      /* byte offset of each plane inside one picture (NV12 / NV21: two planes) */
    int64_t pitch[3];          /* bytes between lines, > 0, at least a line's bytes */
    int64_t picture_stride;    /* bytes between pictures of the clip */
} pcamv_source_t;
int pcamv_gpu_source_check(const pcamv_source_t *src, size_t clip_bytes, int mb_w, int mb_h, int64_t *n_pictures);
int pcamv_gpu_source_picture(const pcamv_source_t *src, const uint8_t *clip, size_t clip_bytes, int64_t picture, int mb_w, int mb_h, uint8_t *const out[3]);
int pcamv_gpu_upload_picture(pcamv_ctx_t *ctx, const pcamv_source_t *src, const uint8_t *clip, size_t clip_bytes, int64_t picture);
int pcamv_gpu_batch_feed_device(pcamv_batch_t *batch, const void *d_clip, int64_t clip_bytes, const pcamv_source_t *src, const int64_t *d_picture, void *stream);
int pcamv_gpu_batch_feed_status(pcamv_batch_t *batch, int32_t *status);
int pcamv_gpu_param_set_head2(const pcamv_stream_params_t *params, int width, int height, int sps_id, int num_ref_frames, int profile_idc, int level_idc,
                              uint8_t *out, size_t cap, size_t *len);
/* diagnostics (tests): the context's own source planes, whole, into out[3] (tight, the coded size), and in *guard_intact (optional)
 * whether the PCAMV_SRC_GUARD bytes behind each of them still hold what pcamv_gpu_open wrote there.  Synchronises */
#define PCAMV_SRC_GUARD 64
int pcamv_gpu_debug_fetch_fenc(pcamv_ctx_t *ctx, uint8_t *const out[3], int *guard_intact);

#ifdef __cplusplus
}
#endif
#endif
