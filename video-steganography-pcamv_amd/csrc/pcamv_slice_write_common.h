/*
 * pcamv_slice_write_common.h -- what the two P-slice writers share (pcamv_slice_write.h: CABAC, pcamv_slice_write_cavlc.h: CAVLC):
 * the output path behind a final byte (sw_emit: emulation prevention, the buffer of SW_OBUF bytes, its stores, the capacity rule),
 * the slice header a caller hands over, the way from a record to a macroblock's final motion and levels (SW_READ_RECORD, sw_block_slot,
 * sw_slot_rank, sw_motion_levels), the capacity bound and the description of a launch (WriteJobs).  Control code that compiles
 * for the device and for the host, under the rules of pcamv_slice_parse.h; included behind pcamv_common.h, a set of primitives and
 * pcamv_logic.h (MBLocal, mb_load, mb_encode).
 */
#ifndef PCAMV_SLICE_WRITE_COMMON_H
#define PCAMV_SLICE_WRITE_COMMON_H
#include "pcamv_slice_parse.h"

#define SW_OBUF 256
/* A capacity no slice exceeds, per macroblock.  CABAC: a decision shifts out at most 6 bits (rangeTabLPS >= 6: renorm shift <= 6), a
 * bypass bin 1.  |level| < 4096 (|residual| <= 255, the core transform's gain is 36, the quantiser's factor at QP 0 is 0.4; chroma DC
 * 16320 * 0.2), so a coefficient is at most significant + last + 14 prefix decisions, 25 bins of Exp-Golomb 0 and a sign: 16 * 6 +
 * 26 = 122 bits, 384 coefficients; 27 coded_block_flags; an mvd component (|mvd| < 2^16) 9 decisions + 33 bins of Exp-Golomb 3 +
 * sign = 88 bits, 32 of them; mb_skip_flag, mb_type 3, sub_mb_type 12, coded_block_pattern 6, mb_qp_delta 1 decisions; the
 * terminal bin 1 bit: 46848 + 162 + 2816 + 23 * 6 + 1 = 49965 bits = 6246 bytes.  (The reference's densest slice seen, QP 0 on
 * saturated noise, has 538 per macroblock: the bound is far from tight, and is no function of the raw picture size.)
 * CAVLC stays far below it.  A residual block is coeff_token (<= 16 bits), a sign per trailing one, a level of at most 28 bits
 * (prefix 15 = 16 bits, a suffix of 12; the Baseline / Main clip allows no longer one) per other coefficient, total_zeros (<= 9)
 * and run_before codes (<= 11 each, and the more zeros the fewer levels): at most 464 bits (SWV_BLK_BITS of
 * pcamv_slice_write_cavlc.h, where it is derived), 26 blocks: 12064 bits.  An mvd component is se(v) of |mvd| <= 2^15 after the
 * wrap to 16 bits: ue(v) of at most 2^16, 33 bits, 32 of them: 1056.  mb_skip_run is ue(v) of at most the picture's macroblocks
 * (< 2^20: 41 bits), mb_type ue(4) 5, four sub_mb_types ue(<= 3) 5 each, coded_block_pattern ue(<= 47) 11, mb_qp_delta 1:
 * 12064 + 1056 + 41 + 5 + 20 + 11 + 1 = 13198 bits = 1650 bytes per macroblock.  The end of the slice is the last mb_skip_run
 * (41 bits), the stop bit and up to 7 zeros: 7 bytes, below SW_TAIL_BOUND. */
#define SW_MB_BOUND 6272
#define SW_TAIL_BOUND 16        /* the flush: 10 bits and the pending byte */

struct SwHeader { const uint8_t *bits; int n_bits, i_frame, nal_byte; };       /* bits: most significant first; nal_byte: nal_ref_idc << 5 | nal_unit_type */

/* The output behind a final byte.  W: a writer's state (SwState, SwvState), which holds
 *   uint8_t *dst; long long cap, n;     n: bytes emitted so far, stored or not
 *   uint32_t *obuf; int fill;           SW_OBUF bytes: byte k is destination byte abase + k; dst + abase is 4-byte aligned
 *   long long abase;
 *   int as_nal, zeros; */

/* ---------------------------------------------------------------- output */
/* what the buffer holds to the destination: whole dwords where all four bytes are the slice's and below cap, single bytes at the ends */
template <class SwAny> PCAMV_DEV void sw_flush(SwAny &W)
{
    uint8_t *d0 = W.dst + W.abase;                   /* 4-byte aligned */
    const long long room = W.cap - W.abase;          /* buffer positions below this may be stored */
    const int lo = W.abase < 0 ? (int)-W.abase : 0, hi = (long long)W.fill < room ? W.fill : (int)(room < 0 ? 0 : room);
    SP_SYNC();
    SP_LANES(l) {
        const int a = 4 * l;
        if (a >= lo && a + 4 <= hi) sp_st32(d0 + a, W.obuf[l]);
        else for (int k = 0; k < 4; k++) if (a + k >= lo && a + k < hi) d0[a + k] = (uint8_t)(W.obuf[l] >> (8 * k));
    }
    SP_SYNC();
    W.abase += W.fill;
    W.fill = 0;
}
template <class SwAny> PCAMV_DEV void sw_raw(SwAny &W, uint32_t b)
{
    if (W.n < W.cap) {
        ((uint8_t *)W.obuf)[W.fill] = (uint8_t)b;
        if (++W.fill == SW_OBUF) sw_flush(W);
    }
    W.n++;
}
/* one final byte of the RBSP */
template <class SwAny> PCAMV_DEV void sw_emit(SwAny &W, uint32_t b)
{
    b &= 255u;
    if (W.as_nal) {
        if (W.zeros == 2 && b <= 3u) { sw_raw(W, 3u); W.zeros = 0; }
        W.zeros = b == 0 ? W.zeros + 1 : 0;
    }
    sw_raw(W, b);
}
/* the start of a slice's output: nothing emitted yet, the buffer laid out like the destination's dwords */
template <class SwAny> PCAMV_DEV void sw_out_begin(SwAny &W, uint8_t *dst, long long cap)
{
    W.dst = dst; W.cap = cap; W.n = 0; W.fill = (int)((uintptr_t)dst & 3u); W.abase = -(long long)W.fill;
    W.as_nal = 0; W.zeros = 0;
}

/* ---------------------------------------------------------------- from a record to motion and levels */
/* the carrier slot (= first block of the partition) that owns block i, and that slot's place among the macroblock's carriers in
 * embedding order: carrier_of_block and carrier_slots of pcamv_logic.h on the four sub-partitions packed in one word, so that a lane
 * indexes no array */
PCAMV_DEV int sw_block_slot(int type, int partition, uint32_t sub, int i)
{
    if (type == PCAMV_P_8x8) {
        const int t = (int)((sub >> (8 * (i >> 2))) & 255u), j = i & 3;
        return (i & 12) + (t == PCAMV_D_L0_8x8 ? 0 : t == PCAMV_D_L0_4x8 ? (j & 1) : t == PCAMV_D_L0_8x4 ? (j & 2) : j);
    }
    if (partition == PCAMV_D_8x16) return sp_blk_x(i) < 2 ? 0 : 4;
    if (partition == PCAMV_D_16x8) return sp_blk_y(i) < 2 ? 0 : 8;
    return 0;
}
PCAMV_DEV int sw_slot_rank(int type, uint32_t sub, int s)
{
    if (type != PCAMV_P_8x8) return s != 0;
    int n = 0;
    for (int k = 0; k < (s >> 2); k++) { const int t = (int)((sub >> (8 * k)) & 255u); n += t == PCAMV_D_L0_8x8 ? 1 : t == PCAMV_D_L0_4x4 ? 4 : 2; }
    const int t = (int)((sub >> (8 * (s >> 2))) & 255u), j = s & 3;
    return n + (t == PCAMV_D_L0_4x4 ? j : j != 0);
}

/* The record r as the writers read it: declares type, partition, sub (the four sub-partitions, one byte each) and used, and makes the
 * calling function return PCAMV_EINVAL / PCAMV_EUNSUP where the record is no P macroblock of this path.  A macro because it declares
 * the caller's four values and returns from the caller. */
#define SW_READ_RECORD(r, type, partition, sub, used) \
    int type = (int)SP_UNI((r)->i_type), partition = (int)SP_UNI((r)->i_partition); \
    const uint32_t sub = SP_UNI((uint32_t)(r)->i_sub_partition[0] | (uint32_t)(r)->i_sub_partition[1] << 8 | (uint32_t)(r)->i_sub_partition[2] << 16 | \
                                (uint32_t)(r)->i_sub_partition[3] << 24); \
    const int used = (int)SP_UNI((r)->used); \
    if (type == PCAMV_P_8x8) { partition = PCAMV_D_8x8; if (sub & 0xfcfcfcfcu) return PCAMV_EINVAL; } \
    else if (type == PCAMV_P_L0) { if (partition != PCAMV_D_16x16 && partition != PCAMV_D_16x8 && partition != PCAMV_D_8x16) return PCAMV_EINVAL; } \
    else if (type != PCAMV_P_SKIP) return PCAMV_EUNSUP

/* A coded macroblock's final motion and its levels.  Motion of the sixteen blocks, one per lane: the record's, each partition's MV
 * from its first block, mv_stego where the flip map says so (flip / car_base / n_car as for sw_run), into the neighbourhood (cmv, cref)
 * and into the primitives' cache.  Levels: prediction from that motion, transform and quantisation as the second pass makes them
 * (mbk_pass2); they are left in L (coef, cdc, nzc, cbp_luma, cbp_chroma). */
PCAMV_DEV void sw_motion_levels(SpState &S, const FrameDev &F, MBLocal *L, const pcamv_mb_t *r, int type, int partition, uint32_t sub, int used,
                                const int8_t *flip, const int *car_base, int n_car, int xy, int mx, int my)
{
    const int base = flip && car_base ? (int)SP_UNI(car_base[xy]) : 0;
    SP_SYNC();
    SP_LANES(i) if (i < 16) {
        const int s = sw_block_slot(type, partition, sub, i), k = base + sw_slot_rank(type, sub, s);
        const int flipped = flip && used && (unsigned)k < (unsigned)n_car && flip[k] == 1;
        const int16_t *m = flipped ? r->mv_stego[s] : r->mv[s];
        S.cmv[sp_s8(i)] = sp_pack(m[0], m[1]); S.cref[sp_s8(i)] = 0;
        L->cmv[scan8_of(i)][0] = m[0]; L->cmv[scan8_of(i)][1] = m[1];
    }
    SP_SYNC();
    mb_load(F, L, mx, my, true);
    L->i_type = type; L->i_partition = partition;
    for (int i = 0; i < 4; i++) L->sub_part[i] = (uint8_t)(sub >> (8 * i));
    prim_load_fenc(F, L);
    mb_encode(F, L, 0, 1);
}

/* the slices of one launch of a writer: slice i goes to bytes[off[i] .. off[i] + cap[i]), its length to len[i], its return code to status[i] */
#define SW_HDR_WORDS 4
struct WriteJobs {
    uint8_t *bytes; long long bytes_size;
    const long long *off, *cap; long long *len; int *status;
    const int *hdr;                     /* n_hdr (1: one for all, or one per slice) entries of SW_HDR_WORDS words {byte offset of the bits behind this
                                         * array's start, n_bits, i_frame, NAL header byte}, then the bits */
    int n_hdr;
    const pcamv_mb_t *mbs;              /* records that hold final motion, uploaded by the caller (a launch of one slice), or NULL: the contexts' own */
    const uint8_t *tab;                 /* SW_TAB_BYTES of pcamv_slice_write.h (k_write_pslice), SV_TAB_BYTES of pcamv_slice_parse_cavlc.h (k_write_pslice_cavlc) */
    uint8_t *scratch; long long scratch_stride;
    int lds_cols, as_nal, final;        /* final: the records with the embedding stage's flip map (else as they are) */
};
#endif
