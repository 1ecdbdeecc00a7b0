/*
 * pcamv_slice_write_cavlc.h -- the CAVLC P-slice writer as control code that compiles for the device and for the host.
 *
 * The --no-cabac counterpart of pcamv_slice_write.h, under the same rules: on the device the body of k_write_pslice_cavlc
 * (pcamv_slice_write_cavlc.hip), one wavefront per slice, control wave-uniform; on the host what
 * tests/emu/slice_write_cavlc_driver.cpp and tests/fuzz/check_slice_write_cavlc.cpp compile with scalar primitives.  No HIP type.
 * Included behind pcamv_common.h, a set of primitives and pcamv_logic.h.
 *
 * What it writes is what the reference's x264_slice_write and x264_macroblock_write_cavlc write for a P slice of this path (H.264
 * 7.3.5, 9.2; frame macroblocks, one reference, 4x4 transform, constant QP): mb_skip_run as ue(v) before every coded macroblock
 * and, when it is not zero, at the slice's end; mb_type ue (0 / 1 / 2 for 16x16 / 16x8 / 8x16; a P_8x8 macroblock as 4,
 * P_8x8ref0, which is what encoder/cavlc.c:431-436 writes when all four references are 0, as they always are here -- the parsers
 * read 3 and 4 alike); the four sub_mb_types; the mvd of every partition as se(v) pairs against sp_predict_mv;
 * coded_block_pattern through the inter mapping; mb_qp_delta se(0) where the pattern is not zero; residual_block_cavlc of the
 * luma 4x4s of the coded 8x8s, the two chroma DC blocks and, where the chroma pattern is 2, the eight chroma AC blocks;
 * rbsp_slice_trailing_bits.
 *
 * Motion, levels and P_SKIP are the CABAC writer's (pcamv_slice_write_common.h: SW_READ_RECORD, sw_motion_levels), and so is its rule
 * that a macroblock the record calls coded is written as coded: the receiver counts carriers per coded macroblock, so a P_L0
 * 16x16 without residual whose MV equals the skip prediction is not folded into P_SKIP.
 *
 * The neighbourhood is the CAVLC parser's (pcamv_slice_parse_cavlc.h, SvState): cnz holds total_coeff, 0x80 = not available, nC
 * is sv_nc_table's, the row buffer has SV_ROW_BYTES per macroblock column (the bottom row's four MVs and eight counts); no mvd
 * cache, no context states, no type of the macroblock above.  The counts of a skipped macroblock, of a macroblock without a
 * pattern and of the blocks a pattern leaves out are 0.  The gather and the hand-on to the next row are restated here, since the
 * parser keeps them inside sv_run.
 *
 * Residual blocks.  A block's bits depend on its own levels and on the counts of its left and upper neighbours only, and the
 * transform stage has every count before the first bit is written.  So lanes 0..25 take one block each, in the lane assignment of
 * prim_cavlc_mb (0..15 luma, 16..23 chroma AC, 24 / 25 chroma DC): first every lane counts its coefficients into cnz, then every
 * lane writes its block's complete bit string -- coeff_token by nC class, the trailing ones' signs, level prefixes and suffixes with
 * the suffix-length adaptation, total_zeros, run_before -- into its own slot of SWV_BLK_DWORDS dwords (most significant bit
 * first), and the string's length beside it.  The lanes read the levels where the transform left them (L->coef, L->cdc) in three
 * descending scans and keep no array of their own.  Then the wave appends the strings of the blocks the pattern codes, in syntax
 * order, to the bit stream, a dword at a time.
 *
 * The code tables are the parser's block (SV_TAB_BYTES, built by sv_build_tables): indexed by symbol, an entry is len | code << 5,
 * which is what an encoder needs; coded_block_pattern -> codeNum is the one entry of its 48 codeNum -> pattern bytes that holds the
 * pattern (one per lane).
 *
 * Level escape (encoder/cavlc.c:64-113, Baseline / Main): where the level code left after the escape offsets is 4096 or more the
 * reference warns ("OVERFLOW levelcode") and writes prefix 15 with the suffix 4094 + sign, the largest magnitude the 12-bit suffix
 * holds.  So does this writer; n_clip counts such codes of a slice.
 *
 * Output: a bit writer.  CAVLC slice data follows the header's last bit directly, with no alignment bits; a 64-bit accumulator
 * hands whole bytes to sw_emit, behind which everything is the CABAC writer's (emulation prevention, the buffer of SW_OBUF bytes,
 * dword stores with byte stores at the ragged ends, nothing stored at or beyond cap, PCAMV_ENOMEM with length 0).
 */
#ifndef PCAMV_SLICE_WRITE_CAVLC_H
#define PCAMV_SLICE_WRITE_CAVLC_H
#include "pcamv_slice_write_common.h"
#include "pcamv_slice_parse_cavlc.h"

/* The longest bit string of one residual block.  coeff_token has at most 16 bits.  A coefficient that is not a trailing one costs
 * at most 28 bits: level_prefix <= 15 (16 bits) and a suffix of 12, the clip above allowing no longer prefix; a trailing one costs
 * 1.  A block of t = 16 coefficients has no total_zeros and no run_before: 16 + 16 * 28 = 464.  With t = 15 there is one zero, so
 * every run_before code is of the table's first row (1 bit), at most 14 of them: 16 + 15 * 28 + 9 (total_zeros) + 14 = 459.
 * With t <= 14 there are t - 1 run_before codes of at most 3 bits, but for runs beyond 6 in the last row, which add a bit per
 * further zero (<= 8): 16 + 28 t + 9 + 3 (t - 1) + 8 = 31 t + 30 <= 464.  Chroma AC (15 positions) and chroma DC (4) have fewer
 * coefficients.  tests/emu/slice_write_cavlc_driver.cpp (swvx_block_bound) maximises over every total, trailing ones, class and
 * placement of zeros with the lengths of the table block and finds 464 / 436 / 118 for luma / chroma AC / chroma DC. */
#define SWV_BLK_BITS 464
#define SWV_BLK_DWORDS 15
#define SWV_NBLK 26
static_assert(SWV_BLK_BITS == 16 + 16 * 28, "coeff_token and sixteen escaped levels");
static_assert(SWV_BLK_BITS <= 32 * SWV_BLK_DWORDS, "a block's bit string fits its slot");

struct SwvState {
    uint8_t *dst; long long cap, n;     /* the output: what sw_emit works on (pcamv_slice_write_common.h) */
    uint32_t *obuf; int fill;
    long long abase;
    int as_nal, zeros;
    SvState S;                          /* the neighbourhood and the tables (S.win and the reader's fields are not used) */
    uint32_t *blk;                      /* [SWV_NBLK][SWV_BLK_DWORDS] the blocks' bit strings, bit 31 of a dword first */
    uint32_t *blen;                     /* [SWV_NBLK] bits of each string | clipped level escapes in it << 16 */
    uint64_t acc; int nacc;             /* bits not yet handed on: the low nacc (< 8 between calls) of acc */
    int bad, n_clip, max_bits, n_fold;  /* for the host drivers: clipped level escapes written, the longest string appended, and P_L0 16x16
                                         * macroblocks without residual on the skip prediction (which the reference would have folded) */
};

/* ---------------------------------------------------------------- bit writer */
PCAMV_DEV void swv_put(SwvState &W, int n, uint32_t v)     /* the low n <= 32 bits of v */
{
    if (n <= 0) return;
    W.acc = (W.acc << n) | (uint64_t)(n < 32 ? v & ((1u << n) - 1u) : v);
    W.nacc += n;
    while (W.nacc >= 8) { W.nacc -= 8; sw_emit(W, (uint32_t)(W.acc >> W.nacc)); }
}
PCAMV_DEV void swv_ue(SwvState &W, uint32_t k)             /* k < 2^32 - 1; an mvd's is at most 2^16: 33 bits */
{
    const int nb = 32 - __builtin_clz(k + 1u);
    swv_put(W, nb - 1, 0);
    swv_put(W, nb, k + 1u);
}
PCAMV_DEV void swv_se(SwvState &W, int v) { swv_ue(W, v > 0 ? 2u * (uint32_t)v - 1u : 2u * (uint32_t)-v); }

/* ---------------------------------------------------------------- one block's bit string, by one lane */
struct SwvBits { uint32_t *slot; uint64_t acc; int nb, w, bad; };
PCAMV_DEV void swv_bput(SwvBits &B, int n, uint32_t v)     /* the low n <= 28 bits of v; at most 31 bits wait in acc */
{
    B.acc = (B.acc << n) | (uint64_t)(v & ((1u << n) - 1u));
    B.nb += n;
    if (B.nb >= 32) {
        B.nb -= 32;
        if (B.w < SWV_BLK_DWORDS) B.slot[B.w] = (uint32_t)(B.acc >> B.nb); else B.bad = 1;
        B.w++;
    }
}
PCAMV_DEV void swv_bvlc(SwvBits &B, uint32_t e) { if (!(e & 31u)) B.bad = 1; swv_bput(B, (int)(e & 31u), e >> 5); }      /* a table entry: len | code << 5 */
/* one level (9.2.2.1 backwards; encoder/cavlc.c:64-113 for the escape): returns the clipped escapes written (0 or 1) */
PCAMV_DEV int swv_level(SwvBits &B, int v, int sl)
{
    int code = 2 * sp_abs(v) - 2 + (v < 0), clip = 0;
    if ((code >> sl) < 14) { swv_bput(B, (code >> sl) + 1, 1); swv_bput(B, sl, (uint32_t)code); return 0; }
    if (sl == 0 && code < 30) { swv_bput(B, 15, 1); swv_bput(B, 4, (uint32_t)(code - 14)); return 0; }
    if (sl > 0 && (code >> sl) == 14) { swv_bput(B, 15, 1); swv_bput(B, sl, (uint32_t)code); return 0; }
    code -= 15 << sl;
    if (sl == 0) code -= 15;
    if (code >= 1 << 12) { code = (1 << 12) - 2 + (code & 1); clip = 1; }      /* the clipped level keeps its sign */
    swv_bput(B, 16, 1);
    swv_bput(B, 12, (uint32_t)code);
    return clip;
}
/* suffixLength behind a level of magnitude a (9.2.2.1) */
PCAMV_DEV int swv_next_suffix(int sl, int a)
{
    if (sl == 0) sl = 1;
    if (a > (3 << (sl - 1)) && sl < 6) sl++;
    return sl;
}
/* residual_block_cavlc of the `count` levels at l (scan order) with coeff_token class tab (0..3 by nC, 4 = chroma DC) into slot;
 * coded: the block has a level (its flag of the transform stage).  Returns bits | clipped escapes << 16. */
PCAMV_DEV uint32_t swv_block(const uint16_t *vlc, uint32_t *slot, const int16_t *l, int count, int tab, int coded, int &bad)
{
    SwvBits B = {slot, 0, 0, 0, 0};
    int total = 0, last = -1, t1 = 0, ones = 1, clips = 0;
    if (coded)
        for (int i = count - 1; i >= 0; i--) {
            const int v = l[i];
            if (!v) continue;
            if (last < 0) last = i;
            total++;
            if (ones && t1 < 3 && sp_abs(v) == 1) t1++; else ones = 0;
        }
    if (!total) swv_bvlc(B, vlc[SV_T_COEFF + 64 * tab + SV_COEFF0_SLOT]);
    else {
        swv_bvlc(B, vlc[SV_T_COEFF + 64 * tab + 4 * (total - 1) + t1]);
        int sl = total > 10 && t1 < 3, k = 0;
        for (int i = last; i >= 0; i--) {
            const int v = l[i];
            if (!v) continue;
            if (k < t1) swv_bput(B, 1, v < 0);
            else {
                /* the first level behind fewer than three trailing ones cannot be +-1: coded one nearer to zero */
                clips += swv_level(B, k == t1 && t1 < 3 ? v - (v < 0 ? -1 : 1) : v, sl);
                sl = swv_next_suffix(sl, sp_abs(v));
            }
            k++;
        }
        int zeros = last + 1 - total;
        if (total < count) swv_bvlc(B, vlc[tab == 4 ? SV_T_TZDC + 4 * (total - 1) + zeros : SV_T_TZ + 16 * (total - 1) + zeros]);
        int pos = last;
        for (int i = 0; i < total - 1 && zeros > 0; i++) {
            int run = 0;
            while (--pos >= 0 && !l[pos]) run++;
            swv_bvlc(B, vlc[SV_T_RB + 16 * (zeros - 1 < 6 ? zeros - 1 : 6) + run]);
            zeros -= run;
        }
    }
    const int bits = 32 * B.w + B.nb;
    if (B.nb) { if (B.w < SWV_BLK_DWORDS) slot[B.w] = (uint32_t)(B.acc << (32 - B.nb)); else B.bad = 1; }
    if (B.bad || bits > SWV_BLK_BITS) bad = 1;
    return (uint32_t)bits | (uint32_t)clips << 16;
}
/* block b's string behind the bits written so far */
PCAMV_DEV void swv_append(SwvState &W, int b)
{
    const uint32_t e = SP_UNI(W.blen[b]);
    const int bits = (int)(e & 0xffffu);
    const uint32_t *s = W.blk + SWV_BLK_DWORDS * b;
    W.n_clip += (int)(e >> 16);
    if (bits > W.max_bits) W.max_bits = bits;
    for (int k = 0; 32 * k < bits && k < SWV_BLK_DWORDS; k++) {
        const int n = bits - 32 * k < 32 ? bits - 32 * k : 32;
        swv_put(W, n, SP_UNI(s[k]) >> (32 - n));
    }
}

/* ---------------------------------------------------------------- macroblock layer (encoder/cavlc.c) */
/* the mvd of the partition whose first block is idx (width blocks wide): its MV is in the cache already */
PCAMV_DEV void swv_mvd(SwvState &W, int idx, int width)
{
    int mvp[2];
    sp_predict_mv(W.S, idx, width, mvp);
    const uint32_t mv = SP_UNI(W.S.cmv[sp_s8(idx)]);
    /* (what a decoder adds to its prediction, modulo 2^16 like the MV itself) */
    swv_se(W, (int16_t)(uint16_t)(sp_mvx(mv) - (int)SP_UNI(mvp[0])));
    swv_se(W, (int16_t)(uint16_t)(sp_mvy(mv) - (int)SP_UNI(mvp[1])));
}

/* Every macroblock of the picture; mbs, flip, car_base, n_car as for the CABAC writer's sw_run */
PCAMV_DEV int swv_run(SwvState &W, const FrameDev &F, MBLocal *L, const pcamv_mb_t *mbs, const int8_t *flip, const int *car_base, int n_car)
{
    SvState &S = W.S;
    const int mb_w = F.mb_w, mb_h = FD(F).mb_h;
    uint32_t skip_run = 0;
    for (int my = 0; my < mb_h; my++)
        for (int mx = 0; mx < mb_w; mx++) {
            const int xy = my * mb_w + mx;
            const bool left = mx > 0, top = my > 0, topleft = left && top, topright = top && mx < mb_w - 1;
            uint8_t *rt = S.row + (size_t)SV_ROW_BYTES * mx;
            /* the neighbourhood, one cache position per lane (the CAVLC parser's gather: pcamv_slice_parse_cavlc.h, sv_run) */
            uint32_t g_mv[SP_SLOTS], g_nz[SP_SLOTS]; int g_ref[SP_SLOTS];
            SP_SYNC();
            SP_LANES(q) if (q < 48) {
                uint32_t mv = 0, nz = 0x80; int ref = -2;
                const int col = q & 7, r = q >> 3;
                if (left && col == 3 && r >= 1 && r <= 4) { mv = S.cmv[q + 4]; nz = S.cnz[q + 4]; ref = 0; }
                if (left && (q == 8 || q == 16 || q == 32 || q == 40)) nz = S.cnz[q + 2];
                if (top && q >= 4 && q < 8) { mv = sp_ld32(rt + SP_ROW_MV + 4 * (q - 4)); nz = rt[SP_ROW_NZ + q - 4]; ref = 0; }
                if (top && (q == 1 || q == 2)) nz = rt[SP_ROW_NZ + 4 + q - 1];
                if (top && (q == 25 || q == 26)) nz = rt[SP_ROW_NZ + 6 + q - 25];
                if (topleft && q == 3) { mv = S.tl[0]; ref = 0; }
                if (topright && q == 8) { mv = sp_ld32(rt + SV_ROW_BYTES + SP_ROW_MV); ref = 0; }
                if (col >= 4 && r >= 1 && r <= 4) nz = 0;
                if ((col == 1 || col == 2) && (r == 1 || r == 2 || r == 4 || r == 5)) nz = 0;
                g_mv[SP_SLOT(q)] = mv; g_nz[SP_SLOT(q)] = nz; g_ref[SP_SLOT(q)] = ref;
            }
            SP_SYNC();
            SP_LANES(q) if (q < 48) { S.cmv[q] = g_mv[SP_SLOT(q)]; S.cnz[q] = (uint8_t)g_nz[SP_SLOT(q)]; S.cref[q] = (int8_t)g_ref[SP_SLOT(q)]; }
            SP_SYNC();

            const pcamv_mb_t *r = mbs + xy;
            SW_READ_RECORD(r, type, partition, sub, used);
            S.partition = type == PCAMV_P_SKIP ? PCAMV_D_16x16 : partition;
            if (type == PCAMV_P_SKIP) {
                int pm[2];
                sp_predict_pskip(S, pm);
                const uint32_t mv = SP_UNI(sp_pack(pm[0], pm[1]));
                SP_SYNC();
                SP_LANES(l) if (l < 16) { S.cmv[sp_s8(l)] = mv; S.cref[sp_s8(l)] = 0; }
                SP_SYNC();
                skip_run++;
            } else {
                sw_motion_levels(S, F, L, r, type, partition, sub, used, flip, car_base, n_car, xy, mx, my);
                const int cbp_luma = (int)SP_UNI(L->cbp_luma) & 15, cbp_chroma = (int)SP_UNI(L->cbp_chroma) & 3;
                swv_ue(W, skip_run);
                skip_run = 0;
                if (type == PCAMV_P_8x8) {
                    swv_ue(W, 4);
                    for (int i = 0; i < 4; i++) {
                        const int t = (int)((sub >> (8 * i)) & 255u);
                        swv_ue(W, t == PCAMV_D_L0_8x8 ? 0 : t == PCAMV_D_L0_8x4 ? 1 : t == PCAMV_D_L0_4x8 ? 2 : 3);
                    }
                    for (int i = 0; i < 4; i++) {
                        const int t = (int)((sub >> (8 * i)) & 255u);
                        if (t == PCAMV_D_L0_8x8) swv_mvd(W, 4 * i, 2);
                        else if (t == PCAMV_D_L0_8x4) { swv_mvd(W, 4 * i, 2); swv_mvd(W, 4 * i + 2, 2); }
                        else if (t == PCAMV_D_L0_4x8) { swv_mvd(W, 4 * i, 1); swv_mvd(W, 4 * i + 1, 1); }
                        else for (int k = 0; k < 4; k++) swv_mvd(W, 4 * i + k, 1);
                    }
                } else if (partition == PCAMV_D_16x16) { swv_ue(W, 0); swv_mvd(W, 0, 4); }
                else if (partition == PCAMV_D_16x8) { swv_ue(W, 1); swv_mvd(W, 0, 4); swv_mvd(W, 8, 4); }
                else { swv_ue(W, 2); swv_mvd(W, 0, 2); swv_mvd(W, 4, 2); }
                /* coded_block_pattern: the codeNum whose pattern this is */
                const int cbp = cbp_luma | cbp_chroma << 4;
#if defined(PCAMV_HOST_EMU)
                if (type == PCAMV_P_L0 && partition == PCAMV_D_16x16 && !cbp) {
                    int pm[2];
                    sp_predict_pskip(S, pm);
                    W.n_fold += S.cmv[sp_s8(0)] == sp_pack(pm[0], pm[1]);
                }
#endif
                uint64_t hits = 0;
                SP_LANES(l) hits |= SV_BALLOT(l < 48 && S.cbp_of[l < 48 ? l : 0] == cbp, l);
                if (!hits) return PCAMV_EINVAL;
                swv_ue(W, (uint32_t)__builtin_ctzll(hits));
                if (cbp) {
                    swv_put(W, 1, 1);                                       /* mb_qp_delta se(0): constant QP */
                    /* every block's count, then every block's bits: a block's left and upper neighbours may be any lane's */
                    int coded[SP_SLOTS];
                    SP_SYNC();
                    SP_LANES(b) if (b < SWV_NBLK) {
                        const bool mine = b < 16 ? ((cbp_luma >> (b >> 2)) & 1) != 0 : b < 24 ? cbp_chroma == 2 : cbp_chroma != 0;
                        const int16_t *l = b < 16 ? L->coef[b] : b < 24 ? L->coef[b] + 1 : L->cdc[b - 24];
                        const int count = b < 16 ? 16 : b < 24 ? 15 : 4;
                        int total = 0;
                        coded[SP_SLOT(b)] = mine && L->nzc[scan8_all_of(b < 24 ? b : b + 1)] != 0;
                        if (coded[SP_SLOT(b)]) for (int i = 0; i < count; i++) total += l[i] != 0;
                        if (b < 24) S.cnz[sp_nzc_pos(b)] = (uint8_t)total;
                    }
                    SP_SYNC();
                    SP_LANES(b) if (b < SWV_NBLK) {
                        const int16_t *l = b < 16 ? L->coef[b] : b < 24 ? L->coef[b] + 1 : L->cdc[b - 24];
                        int bad = 0;
                        W.blen[b] = swv_block(S.vlc, W.blk + SWV_BLK_DWORDS * b, l, b < 16 ? 16 : b < 24 ? 15 : 4,
                                              b < 24 ? sv_nc_table(S, sp_nzc_pos(b)) : 4, coded[SP_SLOT(b)], bad);
                        if (bad) W.blen[b] = 0x8000u;                       /* no string is that long: the walk below sees it */
                    }
                    SP_SYNC();
                    for (int b = 0; b < SWV_NBLK; b++) if (SP_UNI(W.blen[b]) & 0x8000u) W.bad = 1;
                    if (W.bad) return PCAMV_EINVAL;
                    for (int b = 0; b < 16; b++) if ((cbp_luma >> (b >> 2)) & 1) swv_append(W, b);
                    if (cbp_chroma) {
                        swv_append(W, 24); swv_append(W, 25);
                        if (cbp_chroma == 2) for (int b = 16; b < 24; b++) swv_append(W, b);
                    }
                }
            }
            if (W.n > W.cap) return PCAMV_ENOMEM;
            /* what the next macroblocks read: the bottom row into the row buffer once the MV above-left of the next macroblock is out of it */
            const uint32_t next_tl = top ? sp_ld32(rt + SP_ROW_MV + 12) : 0u;
            SP_SYNC();
            SP_LANES(l) {
                if (l < 4) { sp_st32(rt + SP_ROW_MV + 4 * l, S.cmv[36 + l]); rt[SP_ROW_NZ + l] = S.cnz[36 + l]; }
                else if (l < 8) rt[SP_ROW_NZ + l] = S.cnz[l < 6 ? 17 + (l - 4) : 41 + (l - 6)];
            }
            SP_SYNC();
            S.tl[0] = next_tl;
        }
    if (skip_run) swv_ue(W, skip_run);
    /* rbsp_slice_trailing_bits */
    swv_put(W, 1, 1);
    if (W.nacc) swv_put(W, 8 - W.nacc, 0);
    return W.n > W.cap ? PCAMV_ENOMEM : 0;
}

/* One slice of the picture F describes, into dst[0, cap): (as_nal) start code and header byte, the header's bits, the slice data
 * directly behind them; *len_out its length.  W brings the working memory (S.cmv, cref, cnz, row, tl; blk, blen; obuf) and the tables
 * (S.vlc, S.cbp_of).  H.i_frame is not read.  Returns 0, PCAMV_ENOMEM (the slice does not fit: *len_out = 0; nothing was stored at or
 * beyond cap), PCAMV_EINVAL or PCAMV_EUNSUP (records that are no P macroblocks of this path). */
PCAMV_DEV int pcamv_slice_write_cavlc(SwvState &W, const FrameDev &F, MBLocal *L, const pcamv_mb_t *mbs, const int8_t *flip, const int *car_base,
                                      int n_car, const SwHeader &H, int as_nal, uint8_t *dst, long long cap, long long *len_out)
{
    *len_out = 0;
    if (!mbs || !dst || cap < 0 || H.n_bits < 0 || (H.n_bits && !H.bits) || F.mb_w < 1 || FD(F).mb_h < 1 || F.mb_w * FD(F).mb_h > (1 << 20)) return PCAMV_EINVAL;
    SvState &S = W.S;
    SP_SYNC();
    SP_LANES(l) { if (l < 48) { S.cmv[l] = 0; S.cnz[l] = 0x80; S.cref[l] = -2; } if (l == 0) S.tl[0] = 0; }
    SP_SYNC();
    sw_out_begin(W, dst, cap);
    W.acc = 0; W.nacc = 0; W.bad = 0; W.n_clip = 0; W.max_bits = 0; W.n_fold = 0;
    if (as_nal) { sw_raw(W, 0); sw_raw(W, 0); sw_raw(W, 0); sw_raw(W, 1); sw_raw(W, (uint32_t)H.nal_byte & 255u); W.as_nal = 1; }
    for (int k = 0; k < H.n_bits >> 3; k++) swv_put(W, 8, SP_UNI(H.bits[k]));
    if (H.n_bits & 7) swv_put(W, H.n_bits & 7, SP_UNI(H.bits[H.n_bits >> 3]) >> (8 - (H.n_bits & 7)));
    const int rc = swv_run(W, F, L, mbs, flip, car_base, n_car);
    if (rc) return rc;
    if (W.fill) sw_flush(W);
    *len_out = W.n;
    return 0;
}
#endif
