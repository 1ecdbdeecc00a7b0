/*
 * pcamv_slice_write.h -- the CABAC P-slice writer as control code that compiles for the device and for the host.
 *
 * On the device it is the body of k_write_pslice (pcamv_slice.hip.h): one wavefront per slice, control wave-uniform, the lanes doing
 * what is parallel -- the context initialisation, the gather of a macroblock's neighbourhood, the motion of its sixteen blocks,
 * prediction and transform (the primitives of the analysis), the stores of the output buffer.  On the host it is what
 * tests/emu/slice_write_driver.cpp and tests/fuzz/check_slice_write.cpp compile with scalar primitives (pcamv_prims_emu.h).
 * It is included behind pcamv_common.h, a set of primitives and pcamv_logic.h (MBLocal, mb_load, mb_encode).
 *
 * What it writes is what encoder/cabac.c writes for a P slice of this path (H.264 7.3.5, 9.3; frame macroblocks, one reference,
 * 4x4 transform, constant QP, cabac_init_idc 0): end_of_slice 0 before every macroblock but the first, mb_skip_flag, mb_type,
 * sub_mb_type, the mvd of every partition, coded_block_pattern, mb_qp_delta 0 where a block is coded, residual_block_cabac of
 * categories 2 / 3 / 4 in order, the terminal bin and x264_cabac_encode_flush.  The arithmetic coder is common/cabac.c's: low,
 * range, queue, outstanding bytes; a byte is final once a later byte that is not 0xff has been put (sw_putbyte keeps it in `pend`).
 *
 * A macroblock's motion is the record's, each partition's MV taken from its first block (sw_block_slot), mv_stego where the flip
 * map says so; a P_SKIP macroblock's is inferred from the neighbours as written (8.4.1.1), never read.  Its levels are made here
 * from that motion (prim_predict_mb, prim_mb_transform in the `lv` form): they depend on nothing else, and no pass stores them.
 * A macroblock that is not P_SKIP is written as coded whatever it codes: the receiver counts carriers per coded macroblock
 * (k_extract_prepare), so a P_L0 16x16 without residual whose MV equals the skip prediction is NOT folded into P_SKIP as
 * x264_macroblock_encode would (macroblock.c:783-794); the analysis' own walk of the coded macroblock (entropy_commit) does not either.
 *
 * What is shared with the parser (pcamv_slice_parse.h): the working memory of the neighbourhood (SpState: cmv, cmvd, cref, cnz, the
 * row buffer with its SP_ROW_* layout, tl) and its mechanics (sp_gather, sp_hand_on, sp_fill_pskip, sp_partition), the context
 * initialisation (sp_init_contexts), the MV prediction (sp_predict_mv, sp_predict_pskip), the cache geometry (sp_s8, sp_nzc_pos),
 * SP_LANES / SP_SYNC / SP_UNI.
 *
 * Output.  Final bytes go through sw_emit: with as_nal, emulation prevention runs there, on each byte as it becomes final (the rule
 * of x264_nal_encode, common/common.c:679-691, needs the count of zeros before the byte and nothing else: two bits of state, and no
 * second pass over global memory, which a pass of its own over an output of unknown length would be).  Bytes collect in a buffer
 * of SW_OBUF bytes (LDS on the device) laid out like the destination's dwords and leave 64 dwords at a time; the partial dwords at
 * both ends of the slice leave as bytes.  Nothing is stored at or beyond `cap`: a slice that does not fit returns PCAMV_ENOMEM.
 */
#ifndef PCAMV_SLICE_WRITE_H
#define PCAMV_SLICE_WRITE_H
#include "pcamv_slice_write_common.h"

#define SW_NCTX 460
#define SW_CTX_BYTES 464
/* the tables as one block: context initialisers (m, n) of all 460 contexts (the state hash covers them all), transitions, rangeTabLPS */
enum { SW_TAB_INIT = 0, SW_TAB_TRANS = 2 * SW_NCTX, SW_TAB_RLPS = SW_TAB_TRANS + 256, SW_TAB_BYTES = SW_TAB_RLPS + 512 };
/* (SW_OBUF, SW_MB_BOUND, SW_TAIL_BOUND, SwHeader and the output path -- sw_emit -- are pcamv_slice_write_common.h's) */
struct SwState {
    SpState S;                          /* the neighbourhood (S.ctx: SW_CTX_BYTES here; S.win is not used) */
    uint32_t low, range; int queue, outstanding, pend;      /* pend: the last byte put, not final yet (-1: none) */
    uint8_t *dst; long long cap, n;     /* n: bytes emitted so far, stored or not */
    uint32_t *obuf; int fill;           /* SW_OBUF bytes: byte k is destination byte abase + k; dst + abase is 4-byte aligned */
    long long abase;
    int as_nal, zeros, bad;
};

/* ---------------------------------------------------------------- arithmetic coder (common/cabac.c:807-926) */
PCAMV_DEV void sw_putbyte(SwState &W)
{
    if (W.queue < 8) return;
    const uint32_t out = W.low >> (W.queue + 2);
    W.low &= (4u << W.queue) - 1u;
    W.queue -= 8;
    if ((out & 255u) == 255u) { W.outstanding++; return; }
    const uint32_t carry = out >> 8;
    if (W.pend >= 0) sw_emit(W, (uint32_t)W.pend + carry);
    for (; W.outstanding > 0; W.outstanding--) sw_emit(W, carry - 1u);
    W.pend = (int)(out & 255u);
}
PCAMV_DEV void sw_renorm(SwState &W)
{
    if (W.range >= 256u) return;
    const int shift = __builtin_clz(W.range | 1u) - 23;         /* x264_cabac_renorm_shift[range >> 3] */
    W.range <<= shift; W.low <<= shift; W.queue += shift;
    sw_putbyte(W);
}
PCAMV_DEV void sw_decision(SwState &W, int ctx, int b)
{
    const uint32_t s = SP_UNI(W.S.ctx[ctx]) & 127u;
    const uint32_t rlps = SP_UNI(W.S.rlps[(4u * s + ((W.range >> 6) & 3u)) & 511u]);
    W.range -= rlps;
    if ((uint32_t)(b != 0) != (s >> 6)) { W.low += W.range; W.range = rlps; }
    W.S.ctx[ctx] = W.S.trans[(2u * s + (uint32_t)(b != 0)) & 255u];
    sw_renorm(W);
}
PCAMV_DEV void sw_bypass(SwState &W, int b)
{
    W.low <<= 1;
    if (b) W.low += W.range;
    W.queue += 1;
    sw_putbyte(W);
}
PCAMV_DEV void sw_ue_bypass(SwState &W, int exp_bits, int val)       /* 0 <= val < 2^20 */
{
    int k;
    for (k = exp_bits; k < 24 && val >= (1 << k); k++) val -= 1 << k;
    const uint32_t x = ((((uint32_t)1 << (k - exp_bits)) - 1u) << (k + 1)) + (uint32_t)val;
    k = 2 * k + 1 - exp_bits;
    int i = ((k - 1) & 7) + 1;
    do {
        k -= i;
        W.low <<= i;
        W.low += ((x >> k) & 255u) * W.range;
        W.queue += i;
        sw_putbyte(W);
        i = 8;
    } while (k > 0);
}
PCAMV_DEV void sw_terminal0(SwState &W) { W.range -= 2; sw_renorm(W); }
PCAMV_DEV void sw_finish(SwState &W, int i_frame)                   /* x264_cabac_encode_flush */
{
    W.low += W.range - 2;
    W.low |= 1;
    W.low <<= 9;
    W.queue += 9;
    sw_putbyte(W);
    sw_putbyte(W);
    W.low <<= 8 - W.queue;
    W.low |= ((0x35a4e4f5u >> (i_frame & 31)) & 1u) << 10;
    W.queue = 8;
    sw_putbyte(W);
    if (W.pend >= 0) sw_emit(W, (uint32_t)W.pend);
    W.pend = -1;
    for (; W.outstanding > 0; W.outstanding--) sw_emit(W, 255u);
}

/* ---------------------------------------------------------------- macroblock layer (encoder/cabac.c) */
PCAMV_DEV void sw_mvd_cpn(SwState &W, int idx, int l, int mvd)
{
    const int i8 = sp_s8(idx);
    const uint32_t pa = W.S.cmvd[i8 - 1], pb = W.S.cmvd[i8 - 8];
    const int amvd = (int)SP_UNI(l ? sp_abs(sp_mvy(pa)) + sp_abs(sp_mvy(pb)) : sp_abs(sp_mvx(pa)) + sp_abs(sp_mvx(pb)));
    const int a = sp_abs(mvd), base = l ? 47 : 40;
    sw_decision(W, base + (amvd > 2) + (amvd > 32), a != 0);
    if (!a) return;
    for (int i = 1; i < (a < 9 ? a : 9); i++) sw_decision(W, base + (i + 2 < 6 ? i + 2 : 6), 1);
    if (a < 9) sw_decision(W, base + (a + 2 < 6 ? a + 2 : 6), 0);
    else sw_ue_bypass(W, 3, a - 9);
    sw_bypass(W, mvd < 0);
}
/* the mvd of the partition whose first block is idx (width x height blocks): its MV is in the cache already */
PCAMV_DEV void sw_mvd(SwState &W, int idx, int width, int height)
{
    int mvp[2];
    sp_predict_mv(W.S, idx, width, mvp);
    const uint32_t mv = SP_UNI(W.S.cmv[sp_s8(idx)]);
    /* (what a decoder adds to its prediction, modulo 2^16 like the MV itself) */
    const int dx = (int16_t)(uint16_t)(sp_mvx(mv) - (int)SP_UNI(mvp[0])), dy = (int16_t)(uint16_t)(sp_mvy(mv) - (int)SP_UNI(mvp[1]));
    sw_mvd_cpn(W, idx, 0, dx);
    sw_mvd_cpn(W, idx, 1, dy);
    const uint32_t md = sp_pack(dx, dy);
    const int lw = width == 4 ? 2 : width == 2 ? 1 : 0, q0 = sp_s8(idx);
    SP_SYNC();
    SP_LANES(l) {
        const int q = q0 + (l & (width - 1)) + 8 * (l >> lw);
        if (l < width * height && q < 48) W.S.cmvd[q] = md;
    }
    SP_SYNC();
}
/* one residual block: count levels at l in scan order, its coded_block_flag `flag` on context increment inc */
PCAMV_DEV void sw_residual(SwState &W, int cat, const int16_t *l, int count, int inc, int flag)
{
    const int sig_off = cat == 2 ? 134 : cat == 3 ? 149 : 152, last_off = cat == 2 ? 195 : cat == 3 ? 210 : 213;
    const int lvl_off = cat == 2 ? 247 : cat == 3 ? 257 : 266;
    sw_decision(W, 85 + 4 * cat + (inc & 3), flag);
    if (!flag) return;
    int last = count - 1;
    while (last >= 0 && !SP_UNI(l[last])) last--;
    if (last < 0) { W.bad = 1; return; }                                   /* a flag without a level: the transform stage never leaves one */
    for (int i = 0; i < (last + 1 < count - 1 ? last + 1 : count - 1); i++) {
        const int nz = SP_UNI(l[i]) != 0;
        sw_decision(W, sig_off + i, nz);
        if (nz) sw_decision(W, last_off + i, i == last);
    }
    int neq1 = 0, ngt1 = 0;
    for (int i = last; i >= 0; i--) {
        const int v = (int)(int16_t)(uint16_t)SP_UNI((uint16_t)l[i]);
        if (!v) continue;
        const int node = ngt1 ? (3 + ngt1 < 7 ? 3 + ngt1 : 7) : (neq1 < 3 ? neq1 : 3);
        const int c1 = node < 4 ? node + 1 : 0, c2 = node < 4 ? 5 : (node + 2 < 9 ? node + 2 : 9);
        const int am1 = sp_abs(v) - 1, prefix = am1 < 14 ? am1 : 14;
        if (prefix) {
            sw_decision(W, lvl_off + c1, 1);
            for (int q = 0; q < prefix - 1; q++) sw_decision(W, lvl_off + c2, 1);
            if (prefix < 14) sw_decision(W, lvl_off + c2, 0);
            else sw_ue_bypass(W, 0, am1 - 14);
            ngt1++;
        } else { sw_decision(W, lvl_off + c1, 0); neq1++; }
        sw_bypass(W, v < 0);
    }
}

/* Every macroblock of the picture.  mbs: the records; flip / car_base: the embedding stage's flip map in carrier order and each
 * macroblock's first carrier in it (flip == NULL: the records' mv are final); n_car: entries of flip.  hash (optional): FNV-1a of
 * the 460 states after each macroblock. */
PCAMV_DEV int sw_run(SwState &W, const FrameDev &F, MBLocal *L, const pcamv_mb_t *mbs, const int8_t *flip, const int *car_base, int n_car,
                     int i_frame, uint32_t *hash)
{
    SpState &S = W.S;
    const int mb_w = F.mb_w, mb_h = FD(F).mb_h;
    S.cbp_left = 0; S.type_left = 0;
    for (int my = 0; my < mb_h; my++)
        for (int mx = 0; mx < mb_w; mx++) {
            const int xy = my * mb_w + mx;
            const bool left = mx > 0, top = my > 0;
            uint8_t *rt = S.row + (size_t)SP_ROW_BYTES * mx;
            if (xy) sw_terminal0(W);                                        /* end_of_slice_flag 0 of the macroblock before */
            sp_gather(S, rt, left, top, top && mx < mb_w - 1);
            const int cl = left ? S.cbp_left : -1, ct = top ? (int)(rt[SP_ROW_CBP] | rt[SP_ROW_CBP + 1] << 8) : -1;
            const int tl = left ? S.type_left : -1, tt = top ? (int)rt[SP_ROW_TYPE] : -1;

            /* the record: type, partition, sub-partitions; anything else is not a P macroblock of this path */
            const pcamv_mb_t *r = mbs + xy;
            SW_READ_RECORD(r, type, partition, sub, used);
            S.partition = type == PCAMV_P_SKIP ? PCAMV_D_16x16 : partition;
            int cbp_luma = 0, cbp_chroma = 0, dcf = 0;
            if (type != PCAMV_P_SKIP) {
                /* final motion of the sixteen blocks and the levels made from it */
                sw_motion_levels(S, F, L, r, type, partition, sub, used, flip, car_base, n_car, xy, mx, my);
                cbp_luma = (int)SP_UNI(L->cbp_luma) & 15; cbp_chroma = (int)SP_UNI(L->cbp_chroma) & 3;
            }
            const int skip = type == PCAMV_P_SKIP;
            sw_decision(W, 11 + (tl >= 0 && tl != PCAMV_P_SKIP) + (tt >= 0 && tt != PCAMV_P_SKIP), skip);
            if (skip) {
                int pm[2]; sp_fill_pskip(S, pm);
            } else {
                sw_decision(W, 14, 0);
                if (type == PCAMV_P_8x8) { sw_decision(W, 15, 0); sw_decision(W, 16, 1); }
                else if (partition == PCAMV_D_16x16) { sw_decision(W, 15, 0); sw_decision(W, 16, 0); }
                else { sw_decision(W, 15, 1); sw_decision(W, 17, partition == PCAMV_D_16x8); }
                if (type == PCAMV_P_8x8) {
                    for (int i = 0; i < 4; i++) {
                        const int t = (int)((sub >> (8 * i)) & 255u);
                        sw_decision(W, 21, t == PCAMV_D_L0_8x8);
                        if (t != PCAMV_D_L0_8x8) { sw_decision(W, 22, t != PCAMV_D_L0_8x4); if (t != PCAMV_D_L0_8x4) sw_decision(W, 23, t == PCAMV_D_L0_4x8); }
                    }
                }
                for (int k = 0, pt; (pt = sp_partition(type, partition, sub, k)) >= 0; k++) sw_mvd(W, pt & 255, (pt >> 8) & 255, pt >> 16);
                /* coded_block_pattern */
                sw_decision(W, 76 - ((cl >> 1) & 1) - ((ct >> 1) & 2), cbp_luma & 1);
                sw_decision(W, 76 - (cbp_luma & 1) - ((ct >> 2) & 2), (cbp_luma >> 1) & 1);
                sw_decision(W, 76 - ((cl >> 3) & 1) - ((cbp_luma << 1) & 2), (cbp_luma >> 2) & 1);
                sw_decision(W, 76 - ((cbp_luma >> 2) & 1) - (cbp_luma & 2), (cbp_luma >> 3) & 1);
                const int ca = cl & 0x30, cb = ct & 0x30;
                sw_decision(W, 77 + ((ca && cl != -1) ? 1 : 0) + ((cb && ct != -1) ? 2 : 0), cbp_chroma != 0);
                if (cbp_chroma) sw_decision(W, 77 + 4 + (ca == 0x20) + 2 * (cb == 0x20), cbp_chroma > 1);
                if (cbp_luma | cbp_chroma) {
                    sw_decision(W, 60, 0);                                  /* mb_qp_delta 0: constant QP, the last delta was 0 */
                    /* this macroblock's coded_block_flags, all at once: a block's left and upper neighbours come before it */
                    SP_SYNC();
                    SP_LANES(i) if (i < 24) S.cnz[sp_nzc_pos(i)] = (uint8_t)(L->nzc[scan8_all_of(i)] != 0);
                    SP_SYNC();
                    for (int i = 0; i < 16; i++)
                        if ((cbp_luma >> (i >> 2)) & 1) {
                            const int q = sp_nzc_pos(i);
                            sw_residual(W, 2, L->coef[i], 16, (int)SP_UNI((S.cnz[q - 1] != 0) + 2 * (S.cnz[q - 8] != 0)), (int)SP_UNI(S.cnz[q]));
                        }
                    if (cbp_chroma) {
                        for (int k = 0; k < 2; k++) {
                            const int inc = (cl != -1 ? (cl >> (8 + k)) & 1 : 0) + 2 * (ct != -1 ? (ct >> (8 + k)) & 1 : 0);
                            const int f = (int)SP_UNI(L->nzc[scan8_all_of(25 + k)] != 0);
                            sw_residual(W, 3, L->cdc[k], 4, inc, f);
                            dcf |= f << k;
                        }
                        if (cbp_chroma == 2)
                            for (int i = 16; i < 24; i++) {
                                const int q = sp_nzc_pos(i);
                                sw_residual(W, 4, L->coef[i] + 1, 15, (int)SP_UNI((S.cnz[q - 1] != 0) + 2 * (S.cnz[q - 8] != 0)), (int)SP_UNI(S.cnz[q]));
                            }
                    }
                }
                /* (flags of blocks that were not written -- an 8x8 or the chroma AC left out of the pattern -- are zero: the transform
                 * stage clears them with the pattern; a macroblock without a pattern has none) */
                if (!(cbp_luma | cbp_chroma)) { SP_SYNC(); SP_LANES(i) if (i < 24) S.cnz[sp_nzc_pos(i)] = 0; SP_SYNC(); }
                else if (cbp_chroma != 2) { SP_SYNC(); SP_LANES(i) if (i >= 16 && i < 24) S.cnz[sp_nzc_pos(i)] = 0; SP_SYNC(); }
            }
            if (W.bad) return PCAMV_EINVAL;
            if (W.n > W.cap) return PCAMV_ENOMEM;
            /* what the next macroblocks read */
            const int cbp = cbp_luma | cbp_chroma << 4 | dcf << 8;
            sp_hand_on(S, rt, top, cbp, type, nullptr, 0, 0);
            S.cbp_left = cbp; S.type_left = type;
            if (hash) {
                uint32_t h = 2166136261u;
                for (int i = 0; i < SW_NCTX; i++) h = (h ^ S.ctx[i]) * 16777619u;
                SP_LANES(l) if (l == 0) hash[xy] = h;
            }
        }
    sw_finish(W, i_frame);
    return W.n > W.cap ? PCAMV_ENOMEM : 0;
}

/* One slice of the picture F describes, into dst[0, cap): (as_nal) start code and header byte, the header's bits, alignment ones, the
 * slice data; *len_out its length.  W brings the working memory (S.ctx, cmv, cmvd, cref, cnz, row, tl; obuf), T the tables.
 * Returns 0, PCAMV_ENOMEM (the slice does not fit: *len_out = 0; nothing was stored at or beyond cap), PCAMV_EINVAL or PCAMV_EUNSUP
 * (records that are no P macroblocks of this path). */
PCAMV_DEV int pcamv_slice_write(SwState &W, const SpTables &T, const FrameDev &F, MBLocal *L, const pcamv_mb_t *mbs, const int8_t *flip,
                                const int *car_base, int n_car, const SwHeader &H, int as_nal, uint8_t *dst, long long cap,
                                long long *len_out, uint32_t *hash)
{
    *len_out = 0;
    if (!mbs || !dst || cap < 0 || H.n_bits < 0 || (H.n_bits && !H.bits) || F.mb_w < 1) return PCAMV_EINVAL;
    const int qp = FD(F).qp;
    if (qp < 0 || qp > 51) return PCAMV_EINVAL;
    SpState &S = W.S;
    S.trans = T.trans; S.rlps = T.rlps;
    sp_init_contexts(S, T, qp, SW_NCTX);
    SP_LANES(l) { if (l < 48) { S.cmv[l] = 0; S.cmvd[l] = 0; S.cnz[l] = 0; S.cref[l] = -2; } if (l == 0) S.tl[0] = 0; }
    SP_SYNC();
    W.low = 0; W.range = 0x1FE; W.queue = -1; W.outstanding = 0; W.pend = -1; W.bad = 0;
    sw_out_begin(W, dst, cap);
    if (as_nal) { sw_raw(W, 0); sw_raw(W, 0); sw_raw(W, 0); sw_raw(W, 1); sw_raw(W, (uint32_t)H.nal_byte & 255u); W.as_nal = 1; }
    for (int k = 0; k < (H.n_bits + 7) >> 3; k++) {
        uint32_t b = SP_UNI(H.bits[k]);
        if (k == H.n_bits >> 3) b |= 0xffu >> (H.n_bits & 7);           /* cabac_alignment_one_bit up to the byte boundary */
        sw_emit(W, b);
    }
    const int rc = sw_run(W, F, L, mbs, flip, car_base, n_car, H.i_frame, hash);
    if (rc) return rc;
    if (W.fill) sw_flush(W);
    *len_out = W.n;
    return 0;
}

/* (a launch is described by WriteJobs of pcamv_slice_write_common.h) */
#endif
