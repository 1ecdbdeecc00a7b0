/*
 * pcamv_mvsyntax.h -- H.264 MV-syntax extractor: host code of the product library.
 *
 * The payload sits in the motion vectors of the FINAL stream.  The reference has no extractor at all (F6); round 1 checked
 * BER = 0 on the encoder's own record (pass-1 record + flips).  This is the decode side: it parses the slice data of a
 * CABAC-coded P slice the way a decoder does -- arithmetic decoding engine (H.264 9.3.3.2), mb_skip_flag, mb_type,
 * sub_mb_type, mvd, coded_block_pattern, mb_qp_delta and the residual (which has to be decoded to keep the engine in step),
 * MV prediction (8.4.1) -- and returns every macroblock's type, partitioning and motion vectors in the record's layout, from
 * which the carrier LSBs and then the message (pcamv_gpu_stc_extract*) follow.
 *
 * Scope = what this encoder family writes in the P slices of the path: frame macroblocks, one reference picture (ref_idx is
 * not coded), 4x4 transform, cabac_init_idc 0, no intra macroblocks (the fork never picks one in a P frame):
 * anything else is reported as PCAMV_EUNSUP, a stream that does not end where it should as PCAMV_EINVAL.
 * The syntax it mirrors is the one encoder/cabac.c writes (x264_macroblock_write_cabac, x264_cabac_mb_skip, block_residual_
 * write_cabac: 403-470, 540-667, 1000-1018) and pcamv_logic.h sizes (cabac_mb_header); the tables are the standard's
 * (pcamv_entropy_tables.h: context initialisers, state transitions, rangeTabLPS in the 128-state form of common/cabac.c).
 */
#ifndef PCAMV_MVSYNTAX_H
#define PCAMV_MVSYNTAX_H
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace mvsyntax {

struct CabDec {
    const uint8_t *p, *end;
    uint32_t range, offset;
    int bitpos;                 /* bits of *p already consumed */
    int overrun;
    uint8_t state[464];
    int bit()
    {
        if (p >= end) { overrun++; return 0; }
        const int b = (*p >> (7 - bitpos)) & 1;
        if (++bitpos == 8) { bitpos = 0; p++; }
        return b;
    }
    void init(const uint8_t *d, size_t n, int qp)
    {
        p = d; end = d + n; bitpos = 0; overrun = 0;
        pcamv_build_cabac_init(qp, state);
        range = 510; offset = 0;
        for (int i = 0; i < 9; i++) offset = offset << 1 | (uint32_t)bit();
    }
    int decision(int ctx)
    {
        const int s = state[ctx];
        const uint32_t rlps = pcamv_cabac_range_lps[4 * s + ((range >> 6) & 3)];
        int b = s >> 6;
        range -= rlps;
        if (offset >= range) { b ^= 1; offset -= range; range = rlps; }
        state[ctx] = pcamv_cabac_transition[2 * s + b];
        while (range < 256) { range <<= 1; offset = offset << 1 | (uint32_t)bit(); }
        return b;
    }
    int bypass()
    {
        offset = offset << 1 | (uint32_t)bit();
        if (offset >= range) { offset -= range; return 1; }
        return 0;
    }
    int terminal()
    {
        range -= 2;
        if (offset >= range) return 1;
        while (range < 256) { range <<= 1; offset = offset << 1 | (uint32_t)bit(); }
        return 0;
    }
    int ue_bypass(int k)          /* Exp-Golomb suffix of UEGk (9.3.2.3) */
    {
        int v = 0;
        while (bypass()) { v += 1 << k; if (++k > 24) { overrun++; break; } }
        while (k--) v += bypass() << k;
        return v;
    }
};

enum { S8_0 = 4 + 1 * 8 };
static inline int blk_x(int idx) { return (idx & 1) | ((idx >> 1) & 2); }
static inline int blk_y(int idx) { return ((idx >> 1) & 1) | ((idx >> 2) & 2); }
static inline int s8(int idx) { return S8_0 + blk_x(idx) + 8 * blk_y(idx); }
static inline int med3(int a, int b, int c) { const int mn = a < b ? a : b, mx = a < b ? b : a; return mn > c ? mn : (mx < c ? mx : c); }

/* one macroblock's neighbourhood in x264's cache layout (8 columns; row 0 = the line above, column 3 = the column to the left) */
struct MbCache {
    int16_t mv[48][2], mvd[48][2];
    int8_t ref[48];             /* 0 = predicted from the one reference, -2 = not available (outside the picture / not decoded yet) */
    uint8_t nz[48];             /* coded_block_flag of the 4x4 blocks: luma in the motion layout; chroma see nzc_pos */
    int partition;
};
static inline void predict_from3(int ref, int refa, int refb, int refc, const int16_t *a, const int16_t *b, const int16_t *c, int mvp[2])
{
    const int cnt = (refa == ref) + (refb == ref) + (refc == ref);
    if (cnt > 1) { mvp[0] = med3(a[0], b[0], c[0]); mvp[1] = med3(a[1], b[1], c[1]); }
    else if (cnt == 1) { const int16_t *s = refa == ref ? a : refb == ref ? b : c; mvp[0] = s[0]; mvp[1] = s[1]; }
    else if (refb == -2 && refc == -2 && refa != -2) { mvp[0] = a[0]; mvp[1] = a[1]; }
    else { mvp[0] = med3(a[0], b[0], c[0]); mvp[1] = med3(a[1], b[1], c[1]); }
}
/* 8.4.1.3 for the partition whose first 4x4 block is idx, `width` blocks wide (the form of common/macroblock.c:165-231) */
static inline void predict_mv(const MbCache &C, int idx, int width, int mvp[2])
{
    const int i8 = s8(idx), ref = 0;
    int refa = C.ref[i8 - 1], refb = C.ref[i8 - 8], refc = C.ref[i8 - 8 + width];
    const int16_t *a = C.mv[i8 - 1], *b = C.mv[i8 - 8], *c = C.mv[i8 - 8 + width];
    if ((idx & 3) == 3 || (width == 2 && (idx & 3) == 2) || refc == -2) { refc = C.ref[i8 - 8 - 1]; c = C.mv[i8 - 8 - 1]; }
    if (C.partition == PCAMV_D_16x8) {
        if (idx == 0 && refb == ref) { mvp[0] = b[0]; mvp[1] = b[1]; return; }
        if (idx != 0 && refa == ref) { mvp[0] = a[0]; mvp[1] = a[1]; return; }
    } else if (C.partition == PCAMV_D_8x16) {
        if (idx == 0 && refa == ref) { mvp[0] = a[0]; mvp[1] = a[1]; return; }
        if (idx != 0 && refc == ref) { mvp[0] = c[0]; mvp[1] = c[1]; return; }
    }
    predict_from3(ref, refa, refb, refc, a, b, c, mvp);
}
static inline void predict_pskip(const MbCache &C, int mv[2])       /* 8.4.1.1 */
{
    const int refa = C.ref[S8_0 - 1], refb = C.ref[S8_0 - 8];
    const int16_t *a = C.mv[S8_0 - 1], *b = C.mv[S8_0 - 8];
    if (refa == -2 || refb == -2 || !(refa | a[0] | a[1]) || !(refb | b[0] | b[1])) { mv[0] = mv[1] = 0; return; }
    int refc = C.ref[S8_0 - 8 + 4];
    const int16_t *c = C.mv[S8_0 - 8 + 4];
    if (refc == -2) { refc = C.ref[S8_0 - 8 - 1]; c = C.mv[S8_0 - 8 - 1]; }
    predict_from3(0, refa, refb, refc, a, b, c, mv);
}
/* position of the coded_block_flag of block idx (0..15 luma, 16..19 Cb, 20..23 Cr) in MbCache::nz: common/common.h:217-238 */
static inline int nzc_pos(int idx)
{
    if (idx < 16) return s8(idx);
    return 1 + ((idx - 16) & 1) + 8 * (1 + (((idx - 16) >> 1) & 1) + 3 * ((idx - 16) >> 2));
}

struct Parser {
    CabDec d;
    int mb_w, mb_h;
    /* what the following macroblocks read of a decoded one */
    int16_t *fmv, *fmvd;        /* [4 mb_h][4 mb_w][2] */
    uint8_t *fnz;               /* [n_mb][24] coded_block_flags, block order */
    int16_t *fcbp;              /* [n_mb] luma | chroma << 4 | chroma DC flags << 8 (Cb), << 9 (Cr) */
    int8_t *ftype;              /* [n_mb] */
    int last_dqp;

    int mvd_cpn(const MbCache &C, int idx, int l)                       /* encoder/cabac.c:403-449 */
    {
        const int i8 = s8(idx);
        const int amvd = abs(C.mvd[i8 - 1][l]) + abs(C.mvd[i8 - 8][l]);
        const int base = l ? 47 : 40;
        if (!d.decision(base + (amvd > 2) + (amvd > 32))) return 0;
        int a = 1;
        while (a < 9 && d.decision(base + (a + 2 < 6 ? a + 2 : 6))) a++;
        if (a == 9) a += d.ue_bypass(3);
        return d.bypass() ? -a : a;
    }
    void mvd(MbCache &C, int idx, int width, int height)
    {
        int mvp[2];
        predict_mv(C, idx, width, mvp);
        const int dx = mvd_cpn(C, idx, 0), dy = mvd_cpn(C, idx, 1);
        for (int j = 0; j < height; j++)
            for (int i = 0; i < width; i++) {
                const int q = s8(idx) + i + 8 * j;
                C.mv[q][0] = (int16_t)(mvp[0] + dx); C.mv[q][1] = (int16_t)(mvp[1] + dy);
                C.mvd[q][0] = (int16_t)dx; C.mvd[q][1] = (int16_t)dy; C.ref[q] = 0;
            }
    }
    /* one residual block (9.3.2.5-7 as block_residual_write_cabac writes it): returns its coded_block_flag */
    int residual(int cat, int inc)
    {
        static const int sig_off[5] = {105, 120, 134, 149, 152}, last_off[5] = {166, 181, 195, 210, 213}, lvl_off[5] = {227, 237, 247, 257, 266};
        const int cnt = cat == 3 ? 4 : cat == 4 ? 15 : 16;
        if (!d.decision(85 + 4 * cat + inc)) return 0;
        int sig[16], n = 0, i;
        for (i = 0; i < cnt - 1; i++) {
            if (d.decision(sig_off[cat] + i)) {
                sig[n++] = i;
                if (d.decision(last_off[cat] + i)) break;
            }
        }
        if (i == cnt - 1) sig[n++] = i;
        int neq1 = 0, ngt1 = 0;
        for (int k = n - 1; k >= 0; k--) {
            const int node = ngt1 ? (3 + ngt1 < 7 ? 3 + ngt1 : 7) : (neq1 < 3 ? neq1 : 3);
            const int c1 = node < 4 ? node + 1 : 0, c2 = node < 4 ? 5 : (node + 2 < 9 ? node + 2 : 9);
            if (d.decision(lvl_off[cat] + c1)) {
                int prefix = 1;
                while (prefix < 14 && d.decision(lvl_off[cat] + c2)) prefix++;
                if (prefix == 14) d.ue_bypass(0);
                ngt1++;
            } else neq1++;
            d.bypass();                                                 /* sign */
        }
        return 1;
    }

    int run(pcamv_mb_t *out)
    {
        last_dqp = 0;
        for (int my = 0; my < mb_h; my++)
            for (int mx = 0; mx < mb_w; mx++) {
                const int xy = my * mb_w + mx, s4 = 4 * mb_w;
                const bool left = mx > 0, top = my > 0, topleft = left && top, topright = top && mx < mb_w - 1;
                MbCache C;
                memset(&C, 0, sizeof(C));
                memset(C.ref, -2, sizeof(C.ref));
                C.partition = PCAMV_D_16x16;
                auto take = [&](int q, int bx, int by) {                /* neighbour 4x4 block (bx, by) of the picture into cache position q */
                    const int16_t *m = fmv + 2 * (by * s4 + bx), *dd = fmvd + 2 * (by * s4 + bx);
                    C.mv[q][0] = m[0]; C.mv[q][1] = m[1]; C.mvd[q][0] = dd[0]; C.mvd[q][1] = dd[1]; C.ref[q] = 0;
                };
                if (left) for (int j = 0; j < 4; j++) take(S8_0 - 1 + 8 * j, 4 * mx - 1, 4 * my + j);
                if (top) for (int i = 0; i < 4; i++) take(S8_0 - 8 + i, 4 * mx + i, 4 * my - 1);
                if (topleft) take(S8_0 - 8 - 1, 4 * mx - 1, 4 * my - 1);
                if (topright) take(S8_0 - 8 + 4, 4 * mx + 4, 4 * my - 1);
                /* coded_block_flags of the neighbours: not available counts as 0 for an inter macroblock (9.3.3.1.1.9) */
                if (left) { const uint8_t *z = fnz + 24 * (xy - 1);
                    C.nz[nzc_pos(0) - 1] = z[5]; C.nz[nzc_pos(2) - 1] = z[7]; C.nz[nzc_pos(8) - 1] = z[13]; C.nz[nzc_pos(10) - 1] = z[15];
                    C.nz[nzc_pos(16) - 1] = z[17]; C.nz[nzc_pos(18) - 1] = z[19]; C.nz[nzc_pos(20) - 1] = z[21]; C.nz[nzc_pos(22) - 1] = z[23]; }
                if (top) { const uint8_t *z = fnz + 24 * (xy - mb_w);
                    C.nz[nzc_pos(0) - 8] = z[10]; C.nz[nzc_pos(1) - 8] = z[11]; C.nz[nzc_pos(4) - 8] = z[14]; C.nz[nzc_pos(5) - 8] = z[15];
                    C.nz[nzc_pos(16) - 8] = z[18]; C.nz[nzc_pos(17) - 8] = z[19]; C.nz[nzc_pos(20) - 8] = z[22]; C.nz[nzc_pos(21) - 8] = z[23]; }
                const int cl = left ? fcbp[xy - 1] : -1, ct = top ? fcbp[xy - mb_w] : -1;
                const int tl = left ? ftype[xy - 1] : -1, tt = top ? ftype[xy - mb_w] : -1;

                pcamv_mb_t *o = &out[xy];
                memset(o, 0, sizeof(*o));
                for (int i = 0; i < 4; i++) o->i_sub_partition[i] = PCAMV_D_L0_8x8;
                o->i_partition = PCAMV_D_16x16;
                uint8_t sub[4] = {PCAMV_D_L0_8x8, PCAMV_D_L0_8x8, PCAMV_D_L0_8x8, PCAMV_D_L0_8x8};
                int cbp_luma = 0, cbp_chroma = 0, dcf = 0;
                uint8_t nzb[24];
                memset(nzb, 0, sizeof(nzb));
                const int skip = d.decision(11 + (tl >= 0 && tl != PCAMV_P_SKIP) + (tt >= 0 && tt != PCAMV_P_SKIP));
                if (skip) {
                    int mv[2];
                    predict_pskip(C, mv);
                    for (int i = 0; i < 16; i++) { C.mv[s8(i)][0] = (int16_t)mv[0]; C.mv[s8(i)][1] = (int16_t)mv[1]; C.ref[s8(i)] = 0; }
                    o->i_type = PCAMV_P_SKIP;
                    o->pskip_mv[0] = (int16_t)mv[0]; o->pskip_mv[1] = (int16_t)mv[1];
                    last_dqp = 0;
                } else {
                    if (d.decision(14)) return PCAMV_EUNSUP;            /* an intra macroblock in a P slice */
                    if (!d.decision(15)) { if (d.decision(16)) { o->i_type = PCAMV_P_8x8; o->i_partition = PCAMV_D_8x8; } else o->i_type = PCAMV_P_L0; }
                    else { o->i_type = PCAMV_P_L0; o->i_partition = d.decision(17) ? PCAMV_D_16x8 : PCAMV_D_8x16; }
                    C.partition = o->i_partition;
                    if (o->i_type == PCAMV_P_8x8) {
                        for (int i = 0; i < 4; i++) {
                            if (d.decision(21)) sub[i] = PCAMV_D_L0_8x8;
                            else if (!d.decision(22)) sub[i] = PCAMV_D_L0_8x4;
                            else sub[i] = d.decision(23) ? PCAMV_D_L0_4x8 : PCAMV_D_L0_4x4;
                        }
                        for (int i = 0; i < 4; i++)
                            switch (sub[i]) {
                            case PCAMV_D_L0_8x8: mvd(C, 4 * i, 2, 2); break;
                            case PCAMV_D_L0_8x4: mvd(C, 4 * i, 2, 1); mvd(C, 4 * i + 2, 2, 1); break;
                            case PCAMV_D_L0_4x8: mvd(C, 4 * i, 1, 2); mvd(C, 4 * i + 1, 1, 2); break;
                            default: for (int k = 0; k < 4; k++) mvd(C, 4 * i + k, 1, 1); break;
                            }
                        memcpy(o->i_sub_partition, sub, 4);
                    } else if (o->i_partition == PCAMV_D_16x16) mvd(C, 0, 4, 4);
                    else if (o->i_partition == PCAMV_D_16x8) { mvd(C, 0, 4, 2); mvd(C, 8, 4, 2); }
                    else { mvd(C, 0, 2, 4); mvd(C, 4, 2, 4); }
                    /* coded_block_pattern (encoder/cabac.c:300-356) */
                    int b;
                    b = d.decision(76 - ((cl >> 1) & 1) - ((ct >> 1) & 2)); cbp_luma |= b;
                    b = d.decision(76 - (cbp_luma & 1) - ((ct >> 2) & 2)); cbp_luma |= b << 1;
                    b = d.decision(76 - ((cl >> 3) & 1) - ((cbp_luma << 1) & 2)); cbp_luma |= b << 2;
                    b = d.decision(76 - ((cbp_luma >> 2) & 1) - (cbp_luma & 2)); cbp_luma |= b << 3;
                    const int ca = cl & 0x30, cb = ct & 0x30;
                    if (d.decision(77 + ((ca && cl != -1) ? 1 : 0) + ((cb && ct != -1) ? 2 : 0)))
                        cbp_chroma = 1 + d.decision(77 + 4 + (ca == 0x20) + 2 * (cb == 0x20));
                    if (cbp_luma | cbp_chroma) {                        /* mb_qp_delta */
                        int n = 0;
                        if (d.decision(60 + (last_dqp != 0))) { n = 1; while (d.decision(n == 1 ? 62 : 63)) if (++n > 104) return PCAMV_EINVAL; }
                        last_dqp = n ? ((n + 1) >> 1) * ((n & 1) ? 1 : -1) : 0;
                        for (int i = 0; i < 16; i++)
                            if ((cbp_luma >> (i >> 2)) & 1) {
                                const int q = nzc_pos(i);
                                nzb[i] = (uint8_t)residual(2, (C.nz[q - 1] != 0) + 2 * (C.nz[q - 8] != 0));
                                C.nz[q] = nzb[i];
                            }
                        if (cbp_chroma) {
                            for (int k = 0; k < 2; k++) {
                                const int inc = (cl != -1 ? (cl >> (8 + k)) & 1 : 0) + 2 * (ct != -1 ? (ct >> (8 + k)) & 1 : 0);
                                dcf |= residual(3, inc) << k;
                            }
                            if (cbp_chroma == 2)
                                for (int i = 16; i < 24; i++) {
                                    const int q = nzc_pos(i);
                                    nzb[i] = (uint8_t)residual(4, (C.nz[q - 1] != 0) + 2 * (C.nz[q - 8] != 0));
                                    C.nz[q] = nzb[i];
                                }
                        }
                    } else last_dqp = 0;
                }
                /* what the next macroblocks read */
                for (int i = 0; i < 16; i++) {
                    const int bx = 4 * mx + blk_x(i), by = 4 * my + blk_y(i), q = s8(i);
                    fmv[2 * (by * s4 + bx)] = C.mv[q][0]; fmv[2 * (by * s4 + bx) + 1] = C.mv[q][1];
                    fmvd[2 * (by * s4 + bx)] = skip ? 0 : C.mvd[q][0]; fmvd[2 * (by * s4 + bx) + 1] = skip ? 0 : C.mvd[q][1];
                    o->mv[i][0] = C.mv[q][0]; o->mv[i][1] = C.mv[q][1]; o->ref[i] = 0;
                }
                memcpy(fnz + 24 * xy, nzb, 24);
                fcbp[xy] = (int16_t)(cbp_luma | cbp_chroma << 4 | dcf << 8);
                ftype[xy] = (int8_t)o->i_type;
                const int end = d.terminal();
                if (end != (xy == mb_w * mb_h - 1)) return PCAMV_EINVAL;       /* end_of_slice_flag in the wrong place */
                if (d.overrun) return PCAMV_EINVAL;
            }
        return 0;
    }
};

/* ---------------------------------------------------------------- CAVLC form (encoder/cavlc.c) */
struct BitRd {
    const uint8_t *d; size_t nbits, pos; int overrun;
    unsigned peek(int n) const        /* the next n <= 24 bits, zero-filled past the end */
    {
        unsigned v = 0;
        for (int i = 0; i < n; i++) { const size_t q = pos + (size_t)i; v = v << 1 | (q < nbits ? (unsigned)((d[q >> 3] >> (7 - (q & 7))) & 1) : 0u); }
        return v;
    }
    unsigned get(int n) { const unsigned v = peek(n); pos += (size_t)n; if (pos > nbits) overrun++; return v; }
    unsigned ue()
    {
        int z = 0;
        while (!get(1)) if (++z > 24 || overrun) { overrun++; return 0; }
        return ((1u << z) - 1u) + (z ? get(z) : 0u);
    }
    int se() { const unsigned k = ue(); return (k & 1) ? (int)((k + 1) >> 1) : -(int)(k >> 1); }
};

struct ParserV {
    BitRd b;
    int mb_w, mb_h;
    int16_t *fmv; uint8_t *fnz; int8_t *ftype;      /* motion, total_coeff per 4x4 block [n_mb][24], types */
    uint8_t cbp_of[48];                             /* codeNum -> coded_block_pattern (inverse of Table 9-4's inter column) */

    /* one residual block (9.2): returns TotalCoeff.  tab: 0..3 by nC, 4 = chroma DC; maxc: 16, 15 or 4 */
    int residual(int tab, int maxc)
    {
        int total = -1, t1 = 0;
        if (b.peek(pcamv_vlc_coeff0_len[tab]) == pcamv_vlc_coeff0_code[tab]) { b.get(pcamv_vlc_coeff0_len[tab]); return 0; }
        for (int tc = 1; tc <= (tab == 4 ? 4 : 16) && total < 0; tc++)
            for (int tr = 0; tr <= (tc < 3 ? tc : 3); tr++) {
                const int k = tab * 64 + (tc - 1) * 4 + tr, len = pcamv_vlc_coeff_len[k];
                if (len && b.peek(len) == pcamv_vlc_coeff_code[k]) { b.get(len); total = tc; t1 = tr; break; }
            }
        if (total < 0 || total > maxc) { b.overrun++; return 0; }
        int suffix_len = total > 10 && t1 < 3;
        b.get(t1);                                                       /* signs of the trailing ones */
        for (int i = t1; i < total; i++) {
            int prefix = 0;
            while (!b.get(1)) if (++prefix > 31 || b.overrun) { b.overrun++; return 0; }
            const int ssize = (prefix == 14 && suffix_len == 0) ? 4 : (prefix >= 15 ? prefix - 3 : suffix_len);
            int code = ((prefix < 15 ? prefix : 15) << suffix_len) + (ssize ? (int)b.get(ssize) : 0);
            if (prefix >= 15 && suffix_len == 0) code += 15;
            if (prefix >= 16) code += (1 << (prefix - 3)) - 4096;
            if (i == t1 && t1 < 3) code += 2;
            const int a = (code + 2) >> 1;                              /* |level| */
            if (suffix_len == 0) suffix_len = 1;
            if (a > (3 << (suffix_len - 1)) && suffix_len < 6) suffix_len++;
        }
        int zeros = 0;
        if (total < maxc) {
            const unsigned char *len = tab == 4 ? &pcamv_vlc_total_zeros_dc_len[(total - 1) * 4] : &pcamv_vlc_total_zeros_len[(total - 1) * 16];
            const unsigned short *code = tab == 4 ? &pcamv_vlc_total_zeros_dc_code[(total - 1) * 4] : &pcamv_vlc_total_zeros_code[(total - 1) * 16];
            int z, nz = tab == 4 ? 4 : 16;
            for (z = 0; z < nz; z++) if (len[z] && b.peek(len[z]) == code[z]) { b.get(len[z]); break; }
            if (z == nz) { b.overrun++; return 0; }
            zeros = z;
        }
        for (int i = 0; i < total - 1 && zeros > 0; i++) {
            const int zl = zeros - 1 < 6 ? zeros - 1 : 6;
            int r;
            for (r = 0; r < 16; r++) { const int len = pcamv_vlc_run_before_len[zl * 16 + r]; if (len && b.peek(len) == pcamv_vlc_run_before_code[zl * 16 + r]) { b.get(len); break; } }
            if (r == 16 || r > zeros) { b.overrun++; return 0; }
            zeros -= r;
        }
        return total;
    }
    void mvd(MbCache &C, int idx, int width, int height)
    {
        int mvp[2];
        predict_mv(C, idx, width, mvp);
        const int dx = b.se(), dy = b.se();
        for (int j = 0; j < height; j++)
            for (int i = 0; i < width; i++) {
                const int q = s8(idx) + i + 8 * j;
                C.mv[q][0] = (int16_t)(mvp[0] + dx); C.mv[q][1] = (int16_t)(mvp[1] + dy); C.ref[q] = 0;
            }
    }
    int run(pcamv_mb_t *out)
    {
        static const uint8_t ct_index[17] = {0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3};
        for (int i = 0; i < 48; i++) cbp_of[pcamv_inter_cbp_to_golomb[i]] = (uint8_t)i;
        int skip_run = -1;              /* -1: the next thing in the stream is an mb_skip_run */
        for (int my = 0; my < mb_h; my++)
            for (int mx = 0; mx < mb_w; mx++) {
                const int xy = my * mb_w + mx, s4 = 4 * mb_w;
                const bool left = mx > 0, top = my > 0, topleft = left && top, topright = top && mx < mb_w - 1;
                MbCache C;
                memset(&C, 0, sizeof(C));
                memset(C.ref, -2, sizeof(C.ref));
                memset(C.nz, 0x80, sizeof(C.nz));                         /* 0x80: not available (common/macroblock.c:1100-1160) */
                C.partition = PCAMV_D_16x16;
                auto take = [&](int q, int bx, int by) { const int16_t *m = fmv + 2 * (by * s4 + bx); C.mv[q][0] = m[0]; C.mv[q][1] = m[1]; C.ref[q] = 0; };
                if (left) for (int j = 0; j < 4; j++) take(S8_0 - 1 + 8 * j, 4 * mx - 1, 4 * my + j);
                if (top) for (int i = 0; i < 4; i++) take(S8_0 - 8 + i, 4 * mx + i, 4 * my - 1);
                if (topleft) take(S8_0 - 8 - 1, 4 * mx - 1, 4 * my - 1);
                if (topright) take(S8_0 - 8 + 4, 4 * mx + 4, 4 * my - 1);
                if (left) { const uint8_t *z = fnz + 24 * (xy - 1);
                    C.nz[nzc_pos(0) - 1] = z[5]; C.nz[nzc_pos(2) - 1] = z[7]; C.nz[nzc_pos(8) - 1] = z[13]; C.nz[nzc_pos(10) - 1] = z[15];
                    C.nz[nzc_pos(16) - 1] = z[17]; C.nz[nzc_pos(18) - 1] = z[19]; C.nz[nzc_pos(20) - 1] = z[21]; C.nz[nzc_pos(22) - 1] = z[23]; }
                if (top) { const uint8_t *z = fnz + 24 * (xy - mb_w);
                    C.nz[nzc_pos(0) - 8] = z[10]; C.nz[nzc_pos(1) - 8] = z[11]; C.nz[nzc_pos(4) - 8] = z[14]; C.nz[nzc_pos(5) - 8] = z[15];
                    C.nz[nzc_pos(16) - 8] = z[18]; C.nz[nzc_pos(17) - 8] = z[19]; C.nz[nzc_pos(20) - 8] = z[22]; C.nz[nzc_pos(21) - 8] = z[23]; }
                for (int i = 0; i < 24; i++) C.nz[nzc_pos(i)] = 0;
                pcamv_mb_t *o = &out[xy];
                memset(o, 0, sizeof(*o));
                for (int i = 0; i < 4; i++) o->i_sub_partition[i] = PCAMV_D_L0_8x8;
                o->i_partition = PCAMV_D_16x16;
                uint8_t nzb[24];
                memset(nzb, 0, sizeof(nzb));
                if (skip_run < 0) skip_run = (int)b.ue();
                if (skip_run > 0) {
                    skip_run--;
                    int mv[2];
                    predict_pskip(C, mv);
                    for (int i = 0; i < 16; i++) { C.mv[s8(i)][0] = (int16_t)mv[0]; C.mv[s8(i)][1] = (int16_t)mv[1]; }
                    o->i_type = PCAMV_P_SKIP;
                    o->pskip_mv[0] = (int16_t)mv[0]; o->pskip_mv[1] = (int16_t)mv[1];
                    /* (when the run is used up the next macroblock is a coded one: no new run is read before it) */
                } else {
                    skip_run = -1;
                    const unsigned mt = b.ue();
                    if (mt > 4) return PCAMV_EUNSUP;                    /* an intra macroblock in a P slice */
                    uint8_t sub[4] = {PCAMV_D_L0_8x8, PCAMV_D_L0_8x8, PCAMV_D_L0_8x8, PCAMV_D_L0_8x8};
                    if (mt >= 3) {
                        static const uint8_t sub_of[4] = {PCAMV_D_L0_8x8, PCAMV_D_L0_8x4, PCAMV_D_L0_4x8, PCAMV_D_L0_4x4};
                        o->i_type = PCAMV_P_8x8; o->i_partition = PCAMV_D_8x8; C.partition = PCAMV_D_8x8;
                        for (int i = 0; i < 4; i++) { const unsigned st = b.ue(); if (st > 3) return PCAMV_EINVAL; sub[i] = sub_of[st]; }
                        for (int i = 0; i < 4; i++)
                            switch (sub[i]) {
                            case PCAMV_D_L0_8x8: mvd(C, 4 * i, 2, 2); break;
                            case PCAMV_D_L0_8x4: mvd(C, 4 * i, 2, 1); mvd(C, 4 * i + 2, 2, 1); break;
                            case PCAMV_D_L0_4x8: mvd(C, 4 * i, 1, 2); mvd(C, 4 * i + 1, 1, 2); break;
                            default: for (int k = 0; k < 4; k++) mvd(C, 4 * i + k, 1, 1); break;
                            }
                        memcpy(o->i_sub_partition, sub, 4);
                    } else {
                        o->i_type = PCAMV_P_L0;
                        o->i_partition = mt == 0 ? PCAMV_D_16x16 : mt == 1 ? PCAMV_D_16x8 : PCAMV_D_8x16;
                        C.partition = o->i_partition;
                        if (mt == 0) mvd(C, 0, 4, 4);
                        else if (mt == 1) { mvd(C, 0, 4, 2); mvd(C, 8, 4, 2); }
                        else { mvd(C, 0, 2, 4); mvd(C, 4, 2, 4); }
                    }
                    const unsigned cn = b.ue();
                    if (cn > 47) return PCAMV_EINVAL;
                    const int cbp = cbp_of[cn], cbp_luma = cbp & 15, cbp_chroma = cbp >> 4;
                    if (cbp) {
                        b.se();                                         /* mb_qp_delta */
                        for (int i = 0; i < 16; i++)
                            if ((cbp_luma >> (i >> 2)) & 1) {
                                const int q = nzc_pos(i);
                                int nc = C.nz[q - 1] + C.nz[q - 8];
                                if (nc < 0x80) nc = (nc + 1) >> 1;
                                nzb[i] = (uint8_t)residual(ct_index[nc & 0x7f], 16);
                                C.nz[q] = nzb[i];
                            }
                        if (cbp_chroma) {
                            residual(4, 4); residual(4, 4);
                            if (cbp_chroma & 2)
                                for (int i = 16; i < 24; i++) {
                                    const int q = nzc_pos(i);
                                    int nc = C.nz[q - 1] + C.nz[q - 8];
                                    if (nc < 0x80) nc = (nc + 1) >> 1;
                                    nzb[i] = (uint8_t)residual(ct_index[nc & 0x7f], 15);
                                    C.nz[q] = nzb[i];
                                }
                        }
                    }
                }
                for (int i = 0; i < 16; i++) {
                    const int bx = 4 * mx + blk_x(i), by = 4 * my + blk_y(i), q = s8(i);
                    fmv[2 * (by * s4 + bx)] = C.mv[q][0]; fmv[2 * (by * s4 + bx) + 1] = C.mv[q][1];
                    o->mv[i][0] = C.mv[q][0]; o->mv[i][1] = C.mv[q][1]; o->ref[i] = 0;
                }
                memcpy(fnz + 24 * xy, nzb, 24);
                ftype[xy] = (int8_t)o->i_type;
                if (b.overrun) return PCAMV_EINVAL;
            }
        if (skip_run > 0) return PCAMV_EINVAL;       /* the last mb_skip_run claims more macroblocks than the picture has left */
        /* rbsp_slice_trailing_bits: a 1 and zeros up to the byte boundary, within the last byte(s) handed over */
        if (b.pos >= b.nbits || !b.get(1)) return PCAMV_EINVAL;
        while (b.pos < b.nbits) if (b.get(1)) return PCAMV_EINVAL;
        return 0;
    }
};
}   /* namespace mvsyntax */

extern "C" int pcamv_gpu_parse_pslice_cabac(const uint8_t *data, size_t len, int mb_w, int mb_h, int slice_qp, pcamv_mb_t *out_mb)
{
    if (!data || !out_mb || len < 2 || mb_w < 1 || mb_h < 1 || slice_qp < 0 || slice_qp > 51) return PCAMV_EINVAL;
    const size_t n = (size_t)mb_w * mb_h;
    mvsyntax::Parser P;
    P.mb_w = mb_w; P.mb_h = mb_h;
    P.fmv = (int16_t *)calloc(n * 32, sizeof(int16_t)); P.fmvd = (int16_t *)calloc(n * 32, sizeof(int16_t));
    P.fnz = (uint8_t *)calloc(n * 24, 1); P.fcbp = (int16_t *)calloc(n, sizeof(int16_t)); P.ftype = (int8_t *)calloc(n, 1);
    int rc = PCAMV_ENOMEM;
    if (P.fmv && P.fmvd && P.fnz && P.fcbp && P.ftype) {
        P.d.init(data, len, slice_qp);
        rc = P.run(out_mb);
    }
    free(P.fmv); free(P.fmvd); free(P.fnz); free(P.fcbp); free(P.ftype);
    return rc;
}
/* The slice data where a real stream has it: inside a NAL unit (emulation prevention bytes, x264_nal_encode common/common.c:658-690)
 * and behind a slice header of any bit length.  pcamv_gpu_nal_to_rbsp undoes the NAL layer; the _at forms start at a bit of the
 * RBSP: CAVLC slice data follows the header directly, CABAC slice data after cabac_alignment_one_bits up to the byte boundary. */
extern "C" int pcamv_gpu_nal_to_rbsp(const uint8_t *nal, size_t len, uint8_t *rbsp, size_t *rbsp_len, int *nal_ref_idc, int *nal_unit_type)
{
    if (!nal || !rbsp || !rbsp_len) return PCAMV_EINVAL;
    size_t i = 0;
    if (len >= 4 && nal[0] == 0 && nal[1] == 0 && nal[2] == 0 && nal[3] == 1) i = 4;           /* Annex B start code, long or short */
    else if (len >= 3 && nal[0] == 0 && nal[1] == 0 && nal[2] == 1) i = 3;
    if (i >= len || (nal[i] & 0x80)) return PCAMV_EINVAL;                                       /* forbidden_zero_bit */
    if (nal_ref_idc) *nal_ref_idc = (nal[i] >> 5) & 3;
    if (nal_unit_type) *nal_unit_type = nal[i] & 31;
    i++;
    size_t n = 0; int zeros = 0;
    for (; i < len; i++) {
        if (zeros >= 2 && nal[i] == 3) {            /* emulation_prevention_three_byte: dropped */
            if (i + 1 < len && nal[i + 1] > 3) return PCAMV_EINVAL;     /* 00 00 03 xx with xx > 03 does not occur in a NAL unit */
            zeros = 0;
            continue;
        }
        if (zeros >= 2 && nal[i] < 3) return PCAMV_EINVAL;              /* 00 00 00 / 01 / 02 inside a NAL unit: the next start code, not payload */
        zeros = nal[i] == 0 ? zeros + 1 : 0;
        rbsp[n++] = nal[i];
    }
    *rbsp_len = n;
    return 0;
}
extern "C" int pcamv_gpu_parse_pslice_cabac(const uint8_t *data, size_t len, int mb_w, int mb_h, int slice_qp, pcamv_mb_t *out_mb);
extern "C" int pcamv_gpu_parse_pslice_cabac_at(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, int slice_qp, pcamv_mb_t *out_mb)
{
    if (!rbsp || start_bit > len * 8) return PCAMV_EINVAL;
    while (start_bit & 7) {                         /* cabac_alignment_one_bit */
        if (!((rbsp[start_bit >> 3] >> (7 - (start_bit & 7))) & 1)) return PCAMV_EINVAL;
        start_bit++;
    }
    return pcamv_gpu_parse_pslice_cabac(rbsp + (start_bit >> 3), len - (start_bit >> 3), mb_w, mb_h, slice_qp, out_mb);
}
static int parse_pslice_cavlc_bits(const uint8_t *data, size_t len, size_t start_bit, int mb_w, int mb_h, pcamv_mb_t *out_mb);
extern "C" int pcamv_gpu_parse_pslice_cavlc_at(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, pcamv_mb_t *out_mb)
{
    if (!rbsp || start_bit >= len * 8) return PCAMV_EINVAL;
    return parse_pslice_cavlc_bits(rbsp, len, start_bit, mb_w, mb_h, out_mb);
}
extern "C" int pcamv_gpu_parse_pslice_cavlc(const uint8_t *data, size_t len, int mb_w, int mb_h, pcamv_mb_t *out_mb)
{
    return parse_pslice_cavlc_bits(data, len, 0, mb_w, mb_h, out_mb);
}
static int parse_pslice_cavlc_bits(const uint8_t *data, size_t len, size_t start_bit, int mb_w, int mb_h, pcamv_mb_t *out_mb)
{
    if (!data || !out_mb || len < 1 || mb_w < 1 || mb_h < 1) return PCAMV_EINVAL;
    const size_t n = (size_t)mb_w * mb_h;
    mvsyntax::ParserV P;
    P.mb_w = mb_w; P.mb_h = mb_h;
    P.fmv = (int16_t *)calloc(n * 32, sizeof(int16_t)); P.fnz = (uint8_t *)calloc(n * 24, 1); P.ftype = (int8_t *)calloc(n, 1);
    int rc = PCAMV_ENOMEM;
    if (P.fmv && P.fnz && P.ftype) {
        P.b.d = data; P.b.nbits = len * 8; P.b.pos = start_bit; P.b.overrun = 0;
        rc = P.run(out_mb);
    }
    free(P.fmv); free(P.fnz); free(P.ftype);
    return rc;
}
/* The layer above a unit: an Annex B byte stream (H.264 annex B) cut into its NAL units, and the header of a P slice read
 * (slice_header(), 7.3.3, as x264_slice_header_write writes it, encoder/encoder.c:174-305).  These two define what the device does
 * (pcamv_stream_index.h) on every input, valid or not.
 * A start code prefix is any 00 00 01; unit i begins behind the i-th prefix and ends in front of the next one or at len, without its
 * trailing 00 bytes (trailing_zero_8bits, or the zero_byte of a long start code).  units[cap] receives the first cap units, *n_units
 * counts them all, *n_slices those of kind PSLICE or UNSUP.  The kind is read from nal_unit_type and, for type 1, from the first
 * payload byte, which emulation prevention cannot touch: first_mb_in_slice == 0 is its first bit, slice_type the ue behind it. */
static inline int pcamv_unit_kind(int nal_header, int payload0)
{
    if (nal_header < 0) return PCAMV_UNIT_OTHER;
    const int type = nal_header & 31;
    if (type >= 2 && type <= 4) return PCAMV_UNIT_UNSUP;        /* data partitions */
    if (type != 1) return PCAMV_UNIT_OTHER;
    if (payload0 < 0 || !(payload0 & 0x80)) return PCAMV_UNIT_UNSUP;    /* no payload, or first_mb_in_slice != 0 */
    int zeros = 0;
    while (zeros < 7 && !((payload0 << (1 + zeros)) & 0x80)) zeros++;
    if (zeros > 3) return PCAMV_UNIT_UNSUP;                     /* no slice_type there is */
    const int slice_type = (1 << zeros) - 1 + ((payload0 >> (6 - 2 * zeros)) & ((1 << zeros) - 1));
    if (slice_type == 0 || slice_type == 5) return PCAMV_UNIT_PSLICE;
    return slice_type == 2 || slice_type == 7 ? PCAMV_UNIT_OTHER : PCAMV_UNIT_UNSUP;     /* an I slice carries nothing */
}
extern "C" int pcamv_gpu_annexb_index(const uint8_t *bytes, size_t len, pcamv_unit_t *units, size_t cap, int64_t *n_units, int64_t *n_slices)
{
    if ((!bytes && len) || (!units && cap) || !n_units || !n_slices) return PCAMV_EINVAL;
    int64_t nu = 0, ns = 0;
    size_t i = 0, begin = 0;
    int open = 0;
    for (;;) {
        while (i + 2 < len && !(bytes[i] == 0 && bytes[i + 1] == 0 && bytes[i + 2] == 1)) i++;
        const size_t stop = i + 2 < len ? i : len;              /* the next prefix, or the end */
        if (open) {
            size_t end = stop;
            while (end > begin && bytes[end - 1] == 0) end--;
            pcamv_unit_t u;
            u.off = (int64_t)begin; u.len = (int64_t)(end - begin);
            u.nal_header = end > begin ? bytes[begin] : -1;
            u.kind = pcamv_unit_kind(u.nal_header, end > begin + 1 ? bytes[begin + 1] : -1);
            if ((size_t)nu < cap) units[nu] = u;
            nu++;
            if (u.kind != PCAMV_UNIT_OTHER) ns++;
        }
        if (stop == len) break;
        i += 3; begin = i; open = 1;
    }
    *n_units = nu; *n_slices = ns;
    return 0;
}
/* A video cut into its GOPs (the rule: include/pcamv_gpu.h); what k_video_cut does (pcamv_video.h) on every input, valid or not.  The
 * units are walked once with what the rule needs of the past: the nearest VCL unit so far and whether it is an IDR unit */
extern "C" int pcamv_gpu_annexb_gops(const uint8_t *bytes, size_t len, pcamv_gop_t *gops, size_t cap, int64_t *n_gops, int64_t *preamble)
{
    if ((!bytes && len) || (!gops && cap) || !n_gops || !preamble) return PCAMV_EINVAL;
    int64_t nu = 0, ns = 0;
    pcamv_gpu_annexb_index(bytes, len, NULL, 0, &nu, &ns);
    pcamv_unit_t *units = (pcamv_unit_t *)malloc((size_t)(nu ? nu : 1) * sizeof(pcamv_unit_t));
    if (!units) return PCAMV_ENOMEM;
    pcamv_gpu_annexb_index(bytes, len, units, (size_t)nu, &nu, &ns);
    int64_t n = 0, last_vcl = -1, open_off = 0, open_unit = 0;
    for (int64_t u = 0; u < nu; u++) {
        const int type = units[u].nal_header < 0 ? 0 : units[u].nal_header & 31;
        if (type < 1 || type > 5) continue;
        if (type == 5 && (last_vcl < 0 || (units[last_vcl].nal_header & 31) != 5)) {
            const int64_t f = last_vcl + 1, at = f ? units[f - 1].off + units[f - 1].len : 0;
            if (n > 0 && (size_t)(n - 1) < cap) { gops[n - 1].len = at - open_off; gops[n - 1].n_units = f - open_unit; }
            if ((size_t)n < cap) { gops[n].off = at; gops[n].first_unit = f; }
            if (n == 0) *preamble = at;
            open_off = at; open_unit = f;
            n++;
        }
        last_vcl = u;
    }
    if (n > 0 && (size_t)(n - 1) < cap) { gops[n - 1].len = (int64_t)len - open_off; gops[n - 1].n_units = nu - open_unit; }
    if (n == 0) *preamble = (int64_t)len;
    *n_gops = n;
    free(units);
    return 0;
}
namespace mvsyntax {
struct HdrBits {                /* the RBSP bit by bit; past its end every read fails */
    const uint8_t *d; uint64_t nbits, pos; int bad;
    unsigned get1()
    {
        if (pos >= nbits) { bad = 1; return 0; }
        const unsigned b = (d[pos >> 3] >> (7 - (pos & 7))) & 1u;
        pos++;
        return b;
    }
    uint32_t u(int n) { uint32_t v = 0; while (n--) v = v << 1 | get1(); return v; }
    uint64_t ue()
    {
        int zeros = 0;
        while (!bad && !get1()) if (++zeros > 31) bad = 1;
        if (bad) return 0;
        return ((uint64_t)1 << zeros) - 1 + u(zeros);
    }
    int64_t se() { const uint64_t k = ue(); return k & 1 ? (int64_t)((k + 1) >> 1) : -(int64_t)(k >> 1); }
};
}
static inline int pcamv_stream_params_ok(const pcamv_stream_params_t *p)
{
    return p && p->log2_max_frame_num >= 4 && p->log2_max_frame_num <= 16 && p->poc_type >= 0 && p->poc_type <= 2 && p->log2_max_poc_lsb >= 4 &&
           p->log2_max_poc_lsb <= 16 && p->num_ref_idx_l0_default >= 1 && p->num_ref_idx_l0_default <= 32 && p->pic_init_qp >= 0 && p->pic_init_qp <= 51 &&
           p->pps_id >= 0 && p->pps_id <= 255;
}
/* the header of a P slice in rbsp[0, len) (the bytes behind the NAL header byte, unescaped): *start_bit the bit behind it, the number
 * the *_at parsers take; -1 in all three outputs on failure */
extern "C" int pcamv_gpu_parse_slice_header(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                            int32_t *slice_qp, int32_t *frame_num)
{
    if (start_bit) *start_bit = -1;
    if (slice_qp) *slice_qp = -1;
    if (frame_num) *frame_num = -1;
    if ((!rbsp && len) || !start_bit || !slice_qp || !frame_num || !pcamv_stream_params_ok(params) || len > ((size_t)1 << 40)) return PCAMV_EINVAL;
    if (nal_header < 0 || (nal_header & 31) != 1) return PCAMV_EUNSUP;          /* not a coded slice of a non-IDR picture */
    const pcamv_stream_params_t &P = *params;
    mvsyntax::HdrBits b = {rbsp, (uint64_t)len * 8, 0, 0};
    /* a read past the end is PCAMV_EINVAL wherever it happens: looked at after every element, before the element is judged */
#define HDR_EOF() do { if (b.bad) return PCAMV_EINVAL; } while (0)
    if (b.ue() != 0) { HDR_EOF(); return PCAMV_EUNSUP; }                        /* first_mb_in_slice */
    HDR_EOF();
    const uint64_t slice_type = b.ue(); HDR_EOF();
    if (slice_type != 0 && slice_type != 5) return PCAMV_EUNSUP;
    const uint64_t pps_id = b.ue(); HDR_EOF();
    if (pps_id != (uint64_t)P.pps_id) return PCAMV_EUNSUP;
    const uint32_t fn = b.u(P.log2_max_frame_num); HDR_EOF();
    if (P.poc_type == 0) {
        b.u(P.log2_max_poc_lsb); HDR_EOF();
        if (P.pic_order_present) { b.se(); HDR_EOF(); }                         /* delta_pic_order_cnt_bottom */
    } else if (P.poc_type == 1 && !P.delta_pic_order_always_zero) {
        b.se(); HDR_EOF();
        if (P.pic_order_present) { b.se(); HDR_EOF(); }
    }
    if (P.redundant_pic_cnt_present) { b.ue(); HDR_EOF(); }
    uint64_t n_ref = (uint64_t)P.num_ref_idx_l0_default;
    const unsigned over = b.get1(); HDR_EOF();
    if (over) { n_ref = b.ue() + 1; HDR_EOF(); }
    if (n_ref > 1) return PCAMV_EUNSUP;
    const unsigned reorder = b.get1(); HDR_EOF();
    if (reorder)
        for (;;) {
            const uint64_t idc = b.ue(); HDR_EOF();
            if (idc == 3) break;
            if (idc > 3) return PCAMV_EINVAL;
            b.ue(); HDR_EOF();                                                  /* abs_diff_pic_num_minus1 / long_term_pic_num */
        }
    if (P.weighted_pred) return PCAMV_EUNSUP;                                   /* pred_weight_table */
    if ((nal_header >> 5) & 3) {
        const unsigned adaptive = b.get1(); HDR_EOF();
        if (adaptive) return PCAMV_EUNSUP;                                      /* memory management control operations */
    }
    if (P.entropy_cabac) {
        const uint64_t idc = b.ue(); HDR_EOF();
        if (idc != 0) return PCAMV_EUNSUP;                                      /* cabac_init_idc: the parser keeps one table */
    }
    const int64_t qp = P.pic_init_qp + b.se(); HDR_EOF();
    if (qp < 0 || qp > 51) return PCAMV_EINVAL;
    if (P.deblocking_filter_control_present) {
        const uint64_t idc = b.ue(); HDR_EOF();
        if (idc > 2) return PCAMV_EINVAL;
        if (idc != 1) { b.se(); HDR_EOF(); b.se(); HDR_EOF(); }
    }
#undef HDR_EOF
    if (b.pos >= b.nbits) return PCAMV_EINVAL;                                  /* no slice data behind the header */
    *start_bit = (int64_t)b.pos; *slice_qp = (int32_t)qp; *frame_num = (int32_t)fn;
    return 0;
}

/* ---------------------------------------------------------------- the IDR picture of a chain: its slice header read, its I slice decoded
 * The header of an IDR I slice as pcamv_gpu_write_idr_slice_header writes it (csrc/pcamv_idr.h), read in syntax order under the rules of
 * pcamv_gpu_parse_slice_header: nal_unit_type != 5, first_mb_in_slice != 0, slice_type not 2 or 7, pps_id != params->pps_id:
 * PCAMV_EUNSUP; frame_num != 0: PCAMV_EINVAL (7.4.3: an IDR picture's is 0); idr_pic_id above 65535: PCAMV_EINVAL; the POC elements and
 * redundant_pic_cnt are read and not judged; with nal_ref_idc != 0 the two marking flags, long_term_reference_flag 1: PCAMV_EUNSUP;
 * entropy_cabac: PCAMV_EUNSUP (the decoder below reads CAVLC); slice_qp_delta, a QP outside 0 .. 51: PCAMV_EINVAL; without deblocking
 * control, or with an idc that is not 1: PCAMV_EUNSUP (the picture would be filtered), an idc above 2 PCAMV_EINVAL.  A read at or past the
 * end and a ue with more than 31 leading zeros are PCAMV_EINVAL, found before the element is judged.  All three outputs -1 on failure.
 *
 * pcamv_idr_header_parse2 (idc_out given) reads the same header whether or not the picture is filtered: disable_deblocking_filter_idc 0, 1
 * or 2 goes to *idc_out (with one slice per picture 2 filters as 0 does), an idc that is not 1 is followed by the two offsets, either of
 * which non-zero is PCAMV_EUNSUP (the filter here has FilterOffsetA = FilterOffsetB = 0) and outside -6 .. 6 PCAMV_EINVAL; without
 * deblocking control in the PPS nothing is read and the idc is 0 (7.4.3).  Everything before that point is judged as above.
 *
 * first_mb_out given (pcamv_gpu_parse_idr_slice_header3): first_mb_in_slice is read and handed out, up to 2^20 - 1 (above: PCAMV_EINVAL),
 * and not refused; everything else as with idc_out. */
static int pcamv_idr_header_parse2(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                   int32_t *slice_qp, int32_t *idr_pic_id, int32_t *idc_out, int64_t *first_mb_out = NULL)
{
    if (first_mb_out) *first_mb_out = -1;
    if (start_bit) *start_bit = -1;
    if (slice_qp) *slice_qp = -1;
    if (idr_pic_id) *idr_pic_id = -1;
    if (idc_out) *idc_out = -1;
    if ((!rbsp && len) || !start_bit || !slice_qp || !idr_pic_id || !pcamv_stream_params_ok(params) || len > ((size_t)1 << 40)) return PCAMV_EINVAL;
    if (nal_header < 0 || (nal_header & 31) != 5) return PCAMV_EUNSUP;
    const pcamv_stream_params_t &P = *params;
    mvsyntax::HdrBits b = {rbsp, (uint64_t)len * 8, 0, 0};
#define HDR_EOF() do { if (b.bad) return PCAMV_EINVAL; } while (0)
    const uint64_t first_mb = b.ue(); HDR_EOF();
    if (first_mb != 0 && !first_mb_out) return PCAMV_EUNSUP;
    if (first_mb > (1u << 20) - 1) return PCAMV_EINVAL;
    const uint64_t slice_type = b.ue(); HDR_EOF();
    if (slice_type != 2 && slice_type != 7) return PCAMV_EUNSUP;
    const uint64_t pps_id = b.ue(); HDR_EOF();
    if (pps_id != (uint64_t)P.pps_id) return PCAMV_EUNSUP;
    const uint32_t fn = b.u(P.log2_max_frame_num); HDR_EOF();
    if (fn != 0) return PCAMV_EINVAL;
    const uint64_t id = b.ue(); HDR_EOF();
    if (id > 65535) return PCAMV_EINVAL;
    if (P.poc_type == 0) {
        b.u(P.log2_max_poc_lsb); HDR_EOF();
        if (P.pic_order_present) { b.se(); HDR_EOF(); }
    } else if (P.poc_type == 1 && !P.delta_pic_order_always_zero) {
        b.se(); HDR_EOF();
        if (P.pic_order_present) { b.se(); HDR_EOF(); }
    }
    if (P.redundant_pic_cnt_present) { b.ue(); HDR_EOF(); }
    if ((nal_header >> 5) & 3) {
        b.get1(); HDR_EOF();                                                    /* no_output_of_prior_pics_flag */
        const unsigned lt = b.get1(); HDR_EOF();
        if (lt) return PCAMV_EUNSUP;
    }
    if (P.entropy_cabac) return PCAMV_EUNSUP;
    const int64_t qp = P.pic_init_qp + b.se(); HDR_EOF();
    if (qp < 0 || qp > 51) return PCAMV_EINVAL;
    uint64_t idc = 0;
    if (!P.deblocking_filter_control_present) { if (!idc_out) return PCAMV_EUNSUP; }
    else {
        idc = b.ue(); HDR_EOF();
        if (idc > 2) return PCAMV_EINVAL;
        if (!idc_out && idc != 1) return PCAMV_EUNSUP;
        if (idc != 1) {
            const int64_t oa = b.se(); HDR_EOF();
            const int64_t ob = b.se(); HDR_EOF();
            if (oa < -6 || oa > 6 || ob < -6 || ob > 6) return PCAMV_EINVAL;
            if (oa || ob) return PCAMV_EUNSUP;
        }
    }
#undef HDR_EOF
    if (b.pos >= b.nbits) return PCAMV_EINVAL;
    *start_bit = (int64_t)b.pos; *slice_qp = (int32_t)qp; *idr_pic_id = (int32_t)id;
    if (idc_out) *idc_out = (int32_t)idc;
    if (first_mb_out) *first_mb_out = (int64_t)first_mb;
    return 0;
}
extern "C" int pcamv_gpu_parse_idr_slice_header(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                                int32_t *slice_qp, int32_t *idr_pic_id)
{
    return pcamv_idr_header_parse2(rbsp, len, nal_header, params, start_bit, slice_qp, idr_pic_id, NULL);
}
extern "C" int pcamv_gpu_parse_idr_slice_header2(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                                 int32_t *slice_qp, int32_t *idr_pic_id, int32_t *disable_deblocking_filter_idc)
{
    if (!disable_deblocking_filter_idc) {
        if (start_bit) *start_bit = -1;
        if (slice_qp) *slice_qp = -1;
        if (idr_pic_id) *idr_pic_id = -1;
        return PCAMV_EINVAL;
    }
    return pcamv_idr_header_parse2(rbsp, len, nal_header, params, start_bit, slice_qp, idr_pic_id, disable_deblocking_filter_idc);
}
extern "C" int pcamv_gpu_parse_idr_slice_header3(const uint8_t *rbsp, size_t len, int nal_header, const pcamv_stream_params_t *params, int64_t *start_bit,
                                                 int32_t *slice_qp, int32_t *idr_pic_id, int32_t *disable_deblocking_filter_idc, int64_t *first_mb)
{
    if (!disable_deblocking_filter_idc || !first_mb) {
        if (start_bit) *start_bit = -1;
        if (slice_qp) *slice_qp = -1;
        if (idr_pic_id) *idr_pic_id = -1;
        if (disable_deblocking_filter_idc) *disable_deblocking_filter_idc = -1;
        if (first_mb) *first_mb = -1;
        return PCAMV_EINVAL;
    }
    return pcamv_idr_header_parse2(rbsp, len, nal_header, params, start_bit, slice_qp, idr_pic_id, disable_deblocking_filter_idc, first_mb);
}

namespace mvsyntax {
/* A decoder of exactly the I slices the device writes: Intra16x16 macroblocks, CAVLC, one QP, no loop filter (H.264 7.3.5, 8.3.3, 8.3.4,
 * 8.5, 9.2).  Written from the standard alone; with the device's coder (csrc/pcamv_idr.h) it shares the code tables and nothing else.
 * Every read is bounded: BitRd gives zeros past the end and counts the overrun, which fails the macroblock. */
struct IDec {
    BitRd b;
    int mb_w, mb_h, qp, qpc;
    uint8_t *pl[3]; uint8_t *nz;                        /* the planes; total_coeff of the AC blocks [n_mb][24] */

    static int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
    static int vscale(int q6, int i, int j)
    {
        static const int v[6][3] = {{10, 16, 13}, {11, 18, 14}, {13, 20, 16}, {14, 23, 18}, {16, 25, 20}, {18, 29, 23}};
        return v[q6][(i & 1) && (j & 1) ? 1 : !(i & 1) && !(j & 1) ? 0 : 2];
    }
    /* residual_block_cavlc (9.2) into lv[0 .. maxc) in scan order; false on bad data */
    bool residual(int tab, int maxc, int *lv, int *total_out)
    {
        for (int i = 0; i < maxc; i++) lv[i] = 0;
        *total_out = 0;
        int total = -1, t1 = 0;
        if (b.peek(pcamv_vlc_coeff0_len[tab]) == pcamv_vlc_coeff0_code[tab]) { b.get(pcamv_vlc_coeff0_len[tab]); return !b.overrun; }
        for (int tc = 1; tc <= (tab == 4 ? 4 : 16) && total < 0; tc++)
            for (int tr = 0; tr <= (tc < 3 ? tc : 3); tr++) {
                const int k = tab * 64 + (tc - 1) * 4 + tr, len = pcamv_vlc_coeff_len[k];
                if (len && b.peek(len) == pcamv_vlc_coeff_code[k]) { b.get(len); total = tc; t1 = tr; break; }
            }
        if (total < 0 || total > maxc || b.overrun) return false;
        int level[16];
        int suffix_len = total > 10 && t1 < 3;
        for (int i = 0; i < total; i++) {
            if (i < t1) { level[i] = b.get(1) ? -1 : 1; continue; }
            int prefix = 0;
            while (!b.get(1)) if (++prefix > 15 || b.overrun) return false;         /* no prefix above 15 below the High profiles */
            if (b.overrun) return false;
            const int ssize = (prefix == 14 && suffix_len == 0) ? 4 : (prefix == 15 ? 12 : suffix_len);
            int code = ((prefix < 15 ? prefix : 15) << suffix_len) + (ssize ? (int)b.get(ssize) : 0);
            if (prefix == 15 && suffix_len == 0) code += 15;
            if (i == t1 && t1 < 3) code += 2;
            level[i] = code & 1 ? (-code - 1) >> 1 : (code + 2) >> 1;
            const int a = level[i] < 0 ? -level[i] : level[i];
            if (suffix_len == 0) suffix_len = 1;
            if (a > (3 << (suffix_len - 1)) && suffix_len < 6) suffix_len++;
        }
        int zeros = 0;
        if (total < maxc) {
            const unsigned char *len = tab == 4 ? &pcamv_vlc_total_zeros_dc_len[(total - 1) * 4] : &pcamv_vlc_total_zeros_len[(total - 1) * 16];
            const unsigned short *code = tab == 4 ? &pcamv_vlc_total_zeros_dc_code[(total - 1) * 4] : &pcamv_vlc_total_zeros_code[(total - 1) * 16];
            int z, nzc = tab == 4 ? 4 : 16;
            for (z = 0; z < nzc; z++) if (len[z] && b.peek(len[z]) == code[z]) { b.get(len[z]); break; }
            if (z == nzc || z + total > maxc) return false;
            zeros = z;
        }
        int pos = total + zeros - 1;                    /* the place of the last coefficient, which is level[0] */
        for (int i = 0; i < total; i++) {
            if (pos < 0 || pos >= maxc) return false;
            lv[pos] = level[i];
            int run = 0;
            if (i < total - 1 && zeros > 0) {
                const int zl = zeros - 1 < 6 ? zeros - 1 : 6;
                int r;
                for (r = 0; r < 16; r++) { const int len = pcamv_vlc_run_before_len[zl * 16 + r]; if (len && b.peek(len) == pcamv_vlc_run_before_code[zl * 16 + r]) { b.get(len); break; } }
                if (r == 16 || r > zeros) return false;
                run = r; zeros -= r;
            } else if (i == total - 1) run = zeros;
            pos -= 1 + run;
        }
        *total_out = total;
        return !b.overrun;
    }
    static int nc_class(int na, int nb)
    {
        const int nc = na >= 0 && nb >= 0 ? (na + nb + 1) >> 1 : na >= 0 ? na : nb >= 0 ? nb : 0;
        return nc < 2 ? 0 : nc < 4 ? 1 : nc < 8 ? 2 : 3;
    }
    /* 8.5.12 on a block of dequantised coefficients c[i][j], added to the prediction at p (pitch w) */
    static void add_idct(const int c[4][4], uint8_t *p, int w)
    {
        int f[4][4], r[4][4];
        for (int i = 0; i < 4; i++) {
            const int e0 = c[i][0] + c[i][2], e1 = c[i][0] - c[i][2], e2 = (c[i][1] >> 1) - c[i][3], e3 = c[i][1] + (c[i][3] >> 1);
            f[i][0] = e0 + e3; f[i][1] = e1 + e2; f[i][2] = e1 - e2; f[i][3] = e0 - e3;
        }
        for (int j = 0; j < 4; j++) {
            const int g0 = f[0][j] + f[2][j], g1 = f[0][j] - f[2][j], g2 = (f[1][j] >> 1) - f[3][j], g3 = f[1][j] + (f[3][j] >> 1);
            r[0][j] = g0 + g3; r[1][j] = g1 + g2; r[2][j] = g1 - g2; r[3][j] = g0 - g3;
        }
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) p[i * w + j] = (uint8_t)clip8(p[i * w + j] + ((r[i][j] + 32) >> 6));
    }
    /* the prediction of a whole plane block of n x n at (px, py) of plane c: kind 0 DC, 1 horizontal, 2 vertical, 3 plane */
    void predict(int c, int n, int px, int py, int kind, bool left, bool top)
    {
        const int w = (c ? 8 : 16) * mb_w;
        uint8_t *p = pl[c] + (size_t)py * w + px;
        int T[17], L[16];                               /* T[0]: above-left, T[1 + x], L[y] */
        for (int x = -1; x < n; x++) T[1 + x] = top && (x >= 0 || left) ? p[-w + x] : 128;
        for (int y = 0; y < n; y++) L[y] = left ? p[y * w - 1] : 128;
        if (kind == 1) { for (int y = 0; y < n; y++) for (int x = 0; x < n; x++) p[y * w + x] = (uint8_t)L[y]; return; }
        if (kind == 2) { for (int y = 0; y < n; y++) for (int x = 0; x < n; x++) p[y * w + x] = (uint8_t)T[1 + x]; return; }
        if (kind == 3) {
            const int h = n / 2;
            int H = 0, V = 0;
            for (int k = 0; k < h; k++) { H += (k + 1) * (T[1 + h + k] - T[1 + h - 2 - k]); V += (k + 1) * (L[h + k] - (h - 2 - k < 0 ? T[0] : L[h - 2 - k])); }
            const int a = 16 * (L[n - 1] + T[n]), bb = n == 16 ? (5 * H + 32) >> 6 : (34 * H + 32) >> 6, cc = n == 16 ? (5 * V + 32) >> 6 : (34 * V + 32) >> 6;
            for (int y = 0; y < n; y++) for (int x = 0; x < n; x++) p[y * w + x] = (uint8_t)clip8((a + bb * (x - (h - 1)) + cc * (y - (h - 1)) + 16) >> 5);
            return;
        }
        if (n == 16) {
            int st = 0, sl = 0;
            for (int k = 0; k < 16; k++) { st += T[1 + k]; sl += L[k]; }
            const int dc = top && left ? (st + sl + 16) >> 5 : top ? (st + 8) >> 4 : left ? (sl + 8) >> 4 : 128;
            for (int y = 0; y < 16; y++) for (int x = 0; x < 16; x++) p[y * w + x] = (uint8_t)dc;
            return;
        }
        for (int by = 0; by < 2; by++)                  /* 8.3.4.1 .. 8.3.4.3: each 4x4 block of the chroma block has its own DC */
            for (int bx = 0; bx < 2; bx++) {
                int st = 0, sl = 0, dc;
                for (int k = 0; k < 4; k++) { st += T[1 + 4 * bx + k]; sl += L[4 * by + k]; }
                if (bx == by) dc = top && left ? (st + sl + 4) >> 3 : top ? (st + 2) >> 2 : left ? (sl + 2) >> 2 : 128;
                else if (bx) dc = top ? (st + 2) >> 2 : left ? (sl + 2) >> 2 : 128;
                else dc = left ? (sl + 2) >> 2 : top ? (st + 2) >> 2 : 128;
                for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++) p[(4 * by + y) * w + 4 * bx + x] = (uint8_t)dc;
            }
    }
    /* ---- I_NxN macroblocks (flags bit 0): Intra4x4 prediction (8.3.1), the 4x4 residual blocks of 16 (7.3.5.3), the intra column of
     * Table 9-4.  modes: Intra4x4PredMode [n_mb][16] by luma4x4BlkIdx, sixteen 2s for an Intra16x16 macroblock (8.3.1.1) */
    int flags = 0;
    uint8_t *modes = NULL;
    /* Intra4x4PredMode m of the block at (px, py) of the luma plane, in place: 8.3.1.2.1 .. 8.3.1.2.9.  hl / ht / hc / hr: the column to the
     * left, the row above, the corner and the four samples above-right are there; false: the mode needs what is missing */
    bool predict4(int px, int py, int m, bool hl, bool ht, bool hc, bool hr)
    {
        const int w = 16 * mb_w;
        uint8_t *p = pl[0] + (size_t)py * w + px;
        if (((m == 0 || m == 3 || m == 7) && !ht) || ((m == 1 || m == 8) && !hl) || ((m == 4 || m == 5 || m == 6) && !(hl && ht && hc)) || m < 0 || m > 8) return false;
        /* the thirteen neighbours on one line: z[0 .. 3] the left column from the bottom up, z[4] the corner, z[5 .. 12] the row above and
         * above-right, left to right; the diagonal modes filter along it */
        int z[13];
        for (int k = 0; k < 13; k++) z[k] = 128;
        if (hl) for (int y = 0; y < 4; y++) z[3 - y] = p[y * w - 1];
        if (hc) z[4] = p[-w - 1];
        if (ht) { for (int x = 0; x < 4; x++) z[5 + x] = p[-w + x]; for (int x = 4; x < 8; x++) z[5 + x] = hr ? p[-w + x] : p[-w + 3]; }
        auto f3 = [&](int a, int c, int e) { return (z[a] + 2 * z[c] + z[e] + 2) >> 2; };
        auto f2 = [&](int a, int c) { return (z[a] + z[c] + 1) >> 1; };
        int o[4][4];
        if (m == 2) {
            const int st = z[5] + z[6] + z[7] + z[8], sl = z[0] + z[1] + z[2] + z[3];
            const int dc = hl && ht ? (st + sl + 4) >> 3 : hl ? (sl + 2) >> 2 : ht ? (st + 2) >> 2 : 128;
            for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++) o[y][x] = dc;
        }
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++) {
                if (m == 0) o[y][x] = z[5 + x];
                else if (m == 1) o[y][x] = z[3 - y];
                else if (m == 3) o[y][x] = x + y == 6 ? (z[11] + 3 * z[12] + 2) >> 2 : f3(5 + x + y, 6 + x + y, 7 + x + y);
                else if (m == 4) o[y][x] = f3(3 + x - y, 4 + x - y, 5 + x - y);                  /* along the line, around the place x - y of the corner */
                else if (m == 5) {                                                              /* vertical-right: the row above, half a sample per row */
                    const int q = 2 * x - y;
                    o[y][x] = q < -1 ? f3(6 - y, 5 - y, 4 - y) : q == -1 ? f3(3, 4, 5) : q & 1 ? f3(3 + x - (y >> 1), 4 + x - (y >> 1), 5 + x - (y >> 1)) : f2(4 + x - (y >> 1), 5 + x - (y >> 1));
                } else if (m == 6) {                                                            /* horizontal-down: the same along the left column */
                    const int q = 2 * y - x;
                    o[y][x] = q < -1 ? f3(2 + x, 3 + x, 4 + x) : q == -1 ? f3(3, 4, 5) : q & 1 ? f3(5 - y + (x >> 1), 4 - y + (x >> 1), 3 - y + (x >> 1)) : f2(4 - y + (x >> 1), 3 - y + (x >> 1));
                } else if (m == 7) o[y][x] = y & 1 ? f3(5 + x + (y >> 1), 6 + x + (y >> 1), 7 + x + (y >> 1)) : f2(5 + x + (y >> 1), 6 + x + (y >> 1));
                else if (m == 8) {
                    const int q = x + 2 * y, k = 3 - y - (x >> 1);                               /* z[k]: the left sample of row y + (x >> 1) */
                    o[y][x] = q > 5 ? z[0] : q == 5 ? (z[1] + 3 * z[0] + 2) >> 2 : q & 1 ? f3(k, k - 1, k - 2) : f2(k, k - 1);
                }
            }
        for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++) p[y * w + x] = (uint8_t)o[y][x];
        return true;
    }
    int mb_nxn(int mx, int my)
    {
        static const int zz[16][2] = {{0, 0}, {0, 1}, {1, 0}, {2, 0}, {1, 1}, {0, 2}, {0, 3}, {1, 2}, {2, 1}, {3, 0}, {3, 1}, {2, 2}, {1, 3}, {2, 3}, {3, 2}, {3, 3}};
        /* Table 9-4, chroma_format_idc 1, the column of Intra_4x4: codeNum -> coded_block_pattern */
        static const uint8_t cbp_of[48] = {47, 31, 15, 0, 23, 27, 29, 30, 7, 11, 13, 14, 39, 43, 45, 46, 16, 3, 5, 10, 12, 19, 21, 26,
                                           28, 35, 37, 42, 44, 1, 2, 4, 8, 17, 18, 20, 24, 6, 9, 22, 25, 32, 33, 34, 36, 40, 38, 41};
        const int xy = my * mb_w + mx;
        const bool left = mx > 0, top = my > 0, topright = top && mx + 1 < mb_w;
        auto blk_at = [](int x, int y) { return (x & 1) | (y & 1) << 1 | (x & 2) << 1 | (y & 2) << 2; };
        uint8_t *md = modes + (size_t)xy * 16;
        const uint8_t *ml = left ? md - 16 : NULL, *mt = top ? md - 16 * mb_w : NULL;
        for (int bi = 0; bi < 16; bi++) {               /* 8.3.1.1 */
            const int x = blk_x(bi), y = blk_y(bi);
            const int ma = x > 0 ? md[blk_at(x - 1, y)] : ml ? ml[blk_at(3, y)] : -1, mb = y > 0 ? md[blk_at(x, y - 1)] : mt ? mt[blk_at(x, 3)] : -1;
            const int pred = ma < 0 || mb < 0 ? 2 : ma < mb ? ma : mb;
            if (b.get(1)) md[bi] = (uint8_t)pred;
            else { const int rem = (int)b.get(3); md[bi] = (uint8_t)(rem < pred ? rem : rem + 1); }
        }
        const unsigned cmode = b.ue();
        if (b.overrun || cmode > 3) return PCAMV_EINVAL;
        const unsigned code = b.ue();
        if (b.overrun || code > 47) return PCAMV_EINVAL;
        const int cbp_l = cbp_of[code] & 15, cbp_c = cbp_of[code] >> 4;
        if (cbp_l | cbp_c) if (b.se() != 0 || b.overrun) return b.overrun ? PCAMV_EINVAL : PCAMV_EUNSUP;    /* mb_qp_delta: one QP */
        if ((cmode == 1 && !left) || (cmode == 2 && !top) || (cmode == 3 && !(left && top))) return PCAMV_EINVAL;
        uint8_t *cnt = nz + (size_t)xy * 24;
        const uint8_t *cl = left ? cnt - 24 : NULL, *ct = top ? cnt - 24 * mb_w : NULL;
        memset(cnt, 0, 24);
        int lv[16][16], total;
        memset(lv, 0, sizeof(lv));
        for (int bi = 0; bi < 16; bi++) {
            if (!(cbp_l >> (bi >> 2) & 1)) continue;
            const int x = blk_x(bi), y = blk_y(bi);
            const int na = x > 0 ? cnt[blk_at(x - 1, y)] : cl ? cl[blk_at(3, y)] : -1, nb = y > 0 ? cnt[blk_at(x, y - 1)] : ct ? ct[blk_at(x, 3)] : -1;
            if (!residual(nc_class(na, nb), 16, lv[bi], &total)) return PCAMV_EINVAL;
            cnt[bi] = (uint8_t)total;
        }
        int cdc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, cac[2][4][16];
        memset(cac, 0, sizeof(cac));
        if (cbp_c) for (int c = 0; c < 2; c++) if (!residual(4, 4, cdc[c], &total)) return PCAMV_EINVAL;
        if (cbp_c == 2)
            for (int c = 0; c < 2; c++)
                for (int k = 0; k < 4; k++) {
                    const int base = 16 + 4 * c, x = k & 1, y = k >> 1;
                    const int na = x ? cnt[base + 2 * y] : cl ? cl[base + 2 * y + 1] : -1, nb = y ? cnt[base + x] : ct ? ct[base + 2 + x] : -1;
                    if (!residual(nc_class(na, nb), 15, cac[c][k] + 1, &total)) return PCAMV_EINVAL;
                    cnt[base + k] = (uint8_t)total;
                }
        /* luma: block by block, each predicted from what is reconstructed so far (8.3.1.2), its sixteen coefficients through 8.5.12 */
        const int q6 = qp % 6, qd = qp / 6;
        for (int bi = 0; bi < 16; bi++) {
            const int x = blk_x(bi), y = blk_y(bi);
            const bool hl = x > 0 || left, ht = y > 0 || top, hc = x > 0 && y > 0 ? true : x > 0 ? top : y > 0 ? left : left && top;
            /* above-right (6.4.11.4): a block decoded later, or one of the macroblock to the right, is not available */
            const bool hr = y > 0 ? x < 3 && blk_at(x + 1, y - 1) < bi : x < 3 ? top : topright;
            if (!predict4(16 * mx + 4 * x, 16 * my + 4 * y, md[bi], hl, ht, hc, hr)) return PCAMV_EINVAL;
            int c4[4][4];
            for (int i = 0; i < 16; i++) c4[zz[i][0]][zz[i][1]] = lv[bi][i] * vscale(q6, zz[i][0], zz[i][1]) * (1 << qd);
            add_idct(c4, pl[0] + (size_t)(16 * my + 4 * y) * 16 * mb_w + 16 * mx + 4 * x, 16 * mb_w);
        }
        const int c6 = qpc % 6, cd = qpc / 6;
        for (int c = 0; c < 2; c++) {
            predict(1 + c, 8, 8 * mx, 8 * my, (int)cmode, left, top);
            const int *d = cdc[c];
            const int f4[4] = {d[0] + d[1] + d[2] + d[3], d[0] - d[1] + d[2] - d[3], d[0] + d[1] - d[2] - d[3], d[0] - d[1] - d[2] + d[3]};
            for (int k = 0; k < 4; k++) {
                int c4[4][4];
                for (int i = 1; i < 16; i++) c4[zz[i][0]][zz[i][1]] = cac[c][k][i] * vscale(c6, zz[i][0], zz[i][1]) * (1 << cd);
                c4[0][0] = (f4[k] * 16 * vscale(c6, 0, 0) * (1 << cd)) >> 5;
                add_idct(c4, pl[1 + c] + (size_t)(8 * my + 4 * (k >> 1)) * 8 * mb_w + 8 * mx + 4 * (k & 1), 8 * mb_w);
            }
        }
        return b.overrun ? PCAMV_EINVAL : 0;
    }
    int run()
    {
        static const int zz[16][2] = {{0, 0}, {0, 1}, {1, 0}, {2, 0}, {1, 1}, {0, 2}, {0, 3}, {1, 2}, {2, 1}, {3, 0}, {3, 1}, {2, 2}, {1, 3}, {2, 3}, {3, 2}, {3, 3}};
        static const int A[4][4] = {{1, 1, 1, 1}, {1, 1, -1, -1}, {1, -1, -1, 1}, {1, -1, 1, -1}};
        for (int my = 0; my < mb_h; my++)
            for (int mx = 0; mx < mb_w; mx++) {
                const int xy = my * mb_w + mx;
                const bool left = mx > 0, top = my > 0;
                const unsigned mb_type = b.ue();
                if (b.overrun) return PCAMV_EINVAL;
                if (mb_type == 0 && (flags & 1)) {      /* I_NxN, where the caller asked for it */
                    const int rc = mb_nxn(mx, my);
                    if (rc) return rc;
                    continue;
                }
                if (modes) memset(modes + (size_t)xy * 16, 2, 16);
                if (mb_type == 0 || mb_type > 24) return mb_type <= 25 ? PCAMV_EUNSUP : PCAMV_EINVAL;      /* I_NxN, I_PCM: not this subset */
                const int mode = (int)(mb_type - 1) & 3, cbp_c = (int)((mb_type - 1) >> 2) % 3, cbp_l = mb_type > 12 ? 15 : 0;
                const unsigned cmode = b.ue();
                if (b.overrun || cmode > 3) return PCAMV_EINVAL;
                if (b.se() != 0 || b.overrun) return b.overrun ? PCAMV_EINVAL : PCAMV_EUNSUP;              /* mb_qp_delta: one QP */
                /* a mode whose neighbours are missing is bad data (8.3.3, 8.3.4) */
                const int lkind = mode == 0 ? 2 : mode == 1 ? 1 : mode == 2 ? 0 : 3;
                const int kinds[2] = {lkind, (int)cmode};
                for (int k = 0; k < 2; k++) if ((kinds[k] == 1 && !left) || (kinds[k] == 2 && !top) || (kinds[k] == 3 && !(left && top))) return PCAMV_EINVAL;
                uint8_t *cnt = nz + (size_t)xy * 24;
                const uint8_t *cl = left ? cnt - 24 : NULL, *ct = top ? cnt - 24 * mb_w : NULL;
                memset(cnt, 0, 24);
                auto blk_at = [](int x, int y) { return (x & 1) | (y & 1) << 1 | (x & 2) << 1 | (y & 2) << 2; };
                auto luma_nc = [&](int bi) {
                    const int x = blk_x(bi), y = blk_y(bi);
                    const int na = x > 0 ? cnt[blk_at(x - 1, y)] : cl ? cl[blk_at(3, y)] : -1, nb = y > 0 ? cnt[blk_at(x, y - 1)] : ct ? ct[blk_at(x, 3)] : -1;
                    return nc_class(na, nb);
                };
                int dc[16], ac[16][16], total;
                if (!residual(luma_nc(0), 16, dc, &total)) return PCAMV_EINVAL;
                for (int bi = 0; bi < 16; bi++) {
                    ac[bi][0] = 0;
                    for (int i = 1; i < 16; i++) ac[bi][i] = 0;
                    if (cbp_l) {
                        if (!residual(luma_nc(bi), 15, ac[bi] + 1, &total)) return PCAMV_EINVAL;
                        cnt[bi] = (uint8_t)total;
                    }
                }
                int cdc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, cac[2][4][16];
                memset(cac, 0, sizeof(cac));
                if (cbp_c) for (int c = 0; c < 2; c++) if (!residual(4, 4, cdc[c], &total)) return PCAMV_EINVAL;
                if (cbp_c == 2)
                    for (int c = 0; c < 2; c++)
                        for (int k = 0; k < 4; k++) {
                            const int base = 16 + 4 * c, x = k & 1, y = k >> 1;
                            const int na = x ? cnt[base + 2 * y] : cl ? cl[base + 2 * y + 1] : -1, nb = y ? cnt[base + x] : ct ? ct[base + 2 + x] : -1;
                            if (!residual(nc_class(na, nb), 15, cac[c][k] + 1, &total)) return PCAMV_EINVAL;
                            cnt[base + k] = (uint8_t)total;
                        }
                /* luma: prediction, the DCs through 8.5.10, every block through 8.5.12 */
                predict(0, 16, 16 * mx, 16 * my, lkind, left, top);
                int cm[4][4], fm[4][4], t[4][4];
                for (int i = 0; i < 16; i++) cm[zz[i][0]][zz[i][1]] = dc[i];
                for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { t[i][j] = 0; for (int k = 0; k < 4; k++) t[i][j] += A[i][k] * cm[k][j]; }
                for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { fm[i][j] = 0; for (int k = 0; k < 4; k++) fm[i][j] += t[i][k] * A[k][j]; }
                const int q6 = qp % 6, qd = qp / 6;
                for (int bi = 0; bi < 16; bi++) {
                    const int x = blk_x(bi), y = blk_y(bi);
                    int c4[4][4];
                    for (int i = 1; i < 16; i++) c4[zz[i][0]][zz[i][1]] = ac[bi][i] * vscale(q6, zz[i][0], zz[i][1]) * (1 << qd);
                    const int f = fm[y][x] * 16 * vscale(q6, 0, 0);
                    c4[0][0] = qd >= 6 ? f * (1 << (qd - 6)) : (f + (1 << (5 - qd))) >> (6 - qd);
                    add_idct(c4, pl[0] + (size_t)(16 * my + 4 * y) * 16 * mb_w + 16 * mx + 4 * x, 16 * mb_w);
                }
                const int c6 = qpc % 6, cd = qpc / 6;
                for (int c = 0; c < 2; c++) {
                    predict(1 + c, 8, 8 * mx, 8 * my, (int)cmode, left, top);
                    const int *d = cdc[c];
                    const int f4[4] = {d[0] + d[1] + d[2] + d[3], d[0] - d[1] + d[2] - d[3], d[0] + d[1] - d[2] - d[3], d[0] - d[1] - d[2] + d[3]};
                    for (int k = 0; k < 4; k++) {
                        int c4[4][4];
                        for (int i = 1; i < 16; i++) c4[zz[i][0]][zz[i][1]] = cac[c][k][i] * vscale(c6, zz[i][0], zz[i][1]) * (1 << cd);
                        c4[0][0] = (f4[k] * 16 * vscale(c6, 0, 0) * (1 << cd)) >> 5;
                        add_idct(c4, pl[1 + c] + (size_t)(8 * my + 4 * (k >> 1)) * 8 * mb_w + 8 * mx + 4 * (k & 1), 8 * mb_w);
                    }
                }
                if (b.overrun) return PCAMV_EINVAL;
            }
        /* rbsp_slice_trailing_bits: the stop bit, zeros to the end of its byte, nothing but cabac_zero_words-free zeros behind */
        if (b.pos >= b.nbits || !b.get(1)) return PCAMV_EINVAL;
        while (b.pos & 7) if (b.get(1)) return PCAMV_EINVAL;
        while (b.pos < b.nbits) if (b.get(8)) return PCAMV_EINVAL;
        return 0;
    }
};
}
/* y / u / v receive the planes tightly packed (16 mb_w x 16 mb_h, half that twice); on failure their contents are unspecified */
/* ... cavlc2: flags bit 0 set makes it accept I_NxN macroblocks (Intra4x4: 8.3.1, the intra column of Table 9-4, mb_qp_delta only with a
 * pattern, nC across the macroblock types) beside the Intra16x16 ones; other bits PCAMV_EINVAL.  With flags 0 it IS the function above */
extern "C" int pcamv_gpu_decode_islice_cavlc2(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, int slice_qp, int chroma_qp_index_offset, int flags,
                                              uint8_t *y, uint8_t *u, uint8_t *v)
{
    static const uint8_t qpc_tab[52] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                        29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};      /* Table 8-15 */
    if (!rbsp || !y || !u || !v || len < 1 || len > ((size_t)1 << 31) || start_bit >= len * 8 || mb_w < 1 || mb_h < 1 || mb_w > (1 << 16) || mb_h > (1 << 16) ||
        (long long)mb_w * mb_h > (1 << 20) || slice_qp < 0 || slice_qp > 51 || chroma_qp_index_offset < -12 || chroma_qp_index_offset > 12 || (flags & ~1)) return PCAMV_EINVAL;
    mvsyntax::IDec D;
    D.b.d = rbsp; D.b.nbits = len * 8; D.b.pos = start_bit; D.b.overrun = 0;
    D.mb_w = mb_w; D.mb_h = mb_h; D.qp = slice_qp;
    const int qi = slice_qp + chroma_qp_index_offset;
    D.qpc = qpc_tab[qi < 0 ? 0 : qi > 51 ? 51 : qi];
    D.pl[0] = y; D.pl[1] = u; D.pl[2] = v;
    D.nz = (uint8_t *)calloc((size_t)mb_w * mb_h, 24);
    if (!D.nz) return PCAMV_ENOMEM;
    D.flags = flags;
    if (flags & 1) { D.modes = (uint8_t *)malloc((size_t)mb_w * mb_h * 16); if (!D.modes) { free(D.nz); return PCAMV_ENOMEM; } }
    const int rc = D.run();
    free(D.nz); free(D.modes);
    return rc;
}
extern "C" int pcamv_gpu_decode_islice_cavlc(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, int slice_qp, int chroma_qp_index_offset,
                                             uint8_t *y, uint8_t *u, uint8_t *v)
{
    return pcamv_gpu_decode_islice_cavlc2(rbsp, len, start_bit, mb_w, mb_h, slice_qp, chroma_qp_index_offset, 0, y, u, v);
}

/* ---------------------------------------------------------------- the loop filter of such a picture (8.7): the definition
 * A frame picture of one slice, intra macroblocks only (Intra16x16 or, with the 4x4 transform, Intra4x4: bS is 4 on macroblock edges and
 * 3 inside for both), one QP, 4x4 transform, FilterOffsetA = FilterOffsetB = 0, filtered in place
 * on tightly packed planes.  Sequential and naive, as the standard words it: macroblocks in raster order; per macroblock the four
 * vertical luma edges left to right, then the four horizontal ones top to bottom, chroma on luma edges 0 and 2 (its own edges 0 and 4);
 * bS 4 on a macroblock edge whose neighbour lies in the picture, 3 on the inner edges, an edge on the picture's border not filtered.
 * indexA = indexB = qp for luma and, for both chroma planes, the chroma QP of qp + chroma_qp_index_offset by Table 8-15; alpha or beta 0
 * leaves a line alone (8.7.2.2: filterSamplesFlag needs |p0 - q0| < alpha), so no QP threshold beside the tables.  This is what the
 * device's filter (csrc/pcamv_idr_deblock.h) is held to; the two share no code and no table. */
namespace mvsyntax {
struct IDeblock {
    int alpha, beta, tc0;               /* of the plane in hand; tc0: the bS 3 column */
    /* one line of samples across an edge: q at q0, step s between samples (8.7.2.3 for bS < 4, 8.7.2.4 for bS 4) */
    void line(uint8_t *q, ptrdiff_t s, int bs, bool chroma) const
    {
        const int p0 = q[-s], p1 = q[-2 * s], q0 = q[0], q1 = q[s];
        if (abs(p0 - q0) >= alpha || abs(p1 - p0) >= beta || abs(q1 - q0) >= beta) return;
        const int p2 = chroma ? 0 : q[-3 * s], q2 = chroma ? 0 : q[2 * s];
        const bool ap = !chroma && abs(p2 - p0) < beta, aq = !chroma && abs(q2 - q0) < beta;
        if (bs < 4) {
            const int tc = chroma ? tc0 + 1 : tc0 + ap + aq;
            int delta = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3;
            delta = delta < -tc ? -tc : delta > tc ? tc : delta;
            q[-s] = (uint8_t)IDec::clip8(p0 + delta);
            q[0] = (uint8_t)IDec::clip8(q0 - delta);
            if (ap) { int d = ((p2 + ((p0 + q0 + 1) >> 1)) >> 1) - p1; d = d < -tc0 ? -tc0 : d > tc0 ? tc0 : d; q[-2 * s] = (uint8_t)(p1 + d); }
            if (aq) { int d = ((q2 + ((p0 + q0 + 1) >> 1)) >> 1) - q1; d = d < -tc0 ? -tc0 : d > tc0 ? tc0 : d; q[s] = (uint8_t)(q1 + d); }
            return;
        }
        const bool strong = !chroma && abs(p0 - q0) < (alpha >> 2) + 2;
        if (ap && strong) {
            const int p3 = q[-4 * s];
            q[-s] = (uint8_t)((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
            q[-2 * s] = (uint8_t)((p2 + p1 + p0 + q0 + 2) >> 2);
            q[-3 * s] = (uint8_t)((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
        } else q[-s] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
        if (aq && strong) {
            const int q3 = q[3 * s];
            q[0] = (uint8_t)((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
            q[s] = (uint8_t)((p0 + q0 + q1 + q2 + 2) >> 2);
            q[2 * s] = (uint8_t)((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
        } else q[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
    }
};
}
extern "C" int pcamv_gpu_deblock_intra_picture(uint8_t *y, uint8_t *u, uint8_t *v, int mb_w, int mb_h, int qp, int chroma_qp_index_offset)
{
    static const uint8_t qpc_of[52] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                       29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};       /* Table 8-15 */
    static const uint8_t alpha_of[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13,
                                         15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255};   /* Table 8-16 */
    static const uint8_t beta_of[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4,
                                        6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18};
    static const uint8_t tc0_of[52][3] = {                                                                                          /* Table 8-17: bS 1, 2, 3 */
        {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0},
        {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 1, 1}, {0, 1, 1}, {1, 1, 1}, {1, 1, 1}, {1, 1, 1},
        {1, 1, 1}, {1, 1, 2}, {1, 1, 2}, {1, 1, 2}, {1, 1, 2}, {1, 2, 3}, {1, 2, 3}, {2, 2, 3}, {2, 2, 4}, {2, 3, 4}, {2, 3, 4}, {3, 3, 5}, {3, 4, 6},
        {3, 4, 6}, {4, 5, 7}, {4, 5, 8}, {4, 6, 9}, {5, 7, 10}, {6, 8, 11}, {6, 8, 13}, {7, 10, 14}, {8, 11, 16}, {9, 12, 18}, {10, 13, 20}, {11, 15, 23},
        {13, 17, 25}};
    if (!y || !u || !v || mb_w < 1 || mb_h < 1 || mb_w > (1 << 16) || mb_h > (1 << 16) || (long long)mb_w * mb_h > (1 << 20) || qp < 0 || qp > 51 ||
        chroma_qp_index_offset < -12 || chroma_qp_index_offset > 12) return PCAMV_EINVAL;
    const int qi = qp + chroma_qp_index_offset, qpc = qpc_of[qi < 0 ? 0 : qi > 51 ? 51 : qi];
    const mvsyntax::IDeblock L = {alpha_of[qp], beta_of[qp], tc0_of[qp][2]}, Cq = {alpha_of[qpc], beta_of[qpc], tc0_of[qpc][2]};
    const ptrdiff_t lw = (ptrdiff_t)16 * mb_w, cw = (ptrdiff_t)8 * mb_w;
    uint8_t *const cpl[2] = {u, v};
    for (int my = 0; my < mb_h; my++)
        for (int mx = 0; mx < mb_w; mx++)
            for (int dir = 0; dir < 2; dir++)                   /* 0: vertical edges (filtered along rows), 1: horizontal edges */
                for (int e = 0; e < 4; e++) {
                    if (e == 0 && (dir ? my : mx) == 0) continue;
                    const int bs = e ? 3 : 4;
                    for (int k = 0; k < 16; k++) {
                        uint8_t *q = dir == 0 ? y + ((ptrdiff_t)16 * my + k) * lw + 16 * mx + 4 * e : y + ((ptrdiff_t)16 * my + 4 * e) * lw + 16 * mx + k;
                        L.line(q, dir == 0 ? 1 : lw, bs, false);
                    }
                    if (e & 1) continue;
                    for (int c = 0; c < 2; c++)
                        for (int k = 0; k < 8; k++) {
                            uint8_t *q = dir == 0 ? cpl[c] + ((ptrdiff_t)8 * my + k) * cw + 8 * mx + 2 * e : cpl[c] + ((ptrdiff_t)8 * my + 2 * e) * cw + 8 * mx + k;
                            Cq.line(q, dir == 0 ? 1 : cw, bs, true);
                        }
                }
    return 0;
}
/* ---------------------------------------------------------------- an IDR picture of one or several slices: the definition
 * bytes[0, len): Annex B.  Every unit of type 5 is a slice of the picture, in the order of the bytes; units that are no VCL units
 * (delimiters, parameter sets, SEI) are passed over; a VCL unit of another type is PCAMV_EUNSUP.  Each slice's header is read by
 * pcamv_gpu_parse_idr_slice_header3 under params; the slices must be whole macroblock rows (first_mb a multiple of mb_w), in order, behind
 * each other without gap or overlap, the first at 0 and the last up to the picture's end, and agree in QP, idr_pic_id and idc: else
 * PCAMV_EUNSUP (no slice at all: PCAMV_EINVAL).  A slice that begins at row r ends where the next begins; it is decoded by
 * pcamv_gpu_decode_islice_cavlc as a picture of its own rows -- for whole-row slices exactly the availability of 7.4.1.2.1 and 9.2.1:
 * nothing above the slice's first row -- into the picture's planes; unless the idc is 1, the whole picture then goes through
 * pcamv_gpu_deblock_intra_picture (idc 0: slice edges are filtered as any macroblock edge; idc 2 is PCAMV_EUNSUP for more than one slice). */
/* ... picture2: flags as pcamv_gpu_decode_islice_cavlc2's, handed to every slice.  The loop filter needs nothing more: with the 4x4
 * transform bS is 4 on macroblock edges and 3 inside for every intra macroblock, Intra4x4 as Intra16x16 */
extern "C" int pcamv_gpu_decode_idr_picture2(const uint8_t *bytes, size_t len, int mb_w, int mb_h, const pcamv_stream_params_t *params, int chroma_qp_index_offset, int flags,
                                             uint8_t *y, uint8_t *u, uint8_t *v, int32_t *slice_qp, int32_t *idr_pic_id, int32_t *n_slices)
{
    if (slice_qp) *slice_qp = -1;
    if (idr_pic_id) *idr_pic_id = -1;
    if (n_slices) *n_slices = 0;
    if (!bytes || !y || !u || !v || !slice_qp || !idr_pic_id || !n_slices || !pcamv_stream_params_ok(params) || len < 1 || len > ((size_t)1 << 31) || mb_w < 1 ||
        mb_h < 1 || mb_w > (1 << 16) || mb_h > (1 << 16) || (long long)mb_w * mb_h > (1 << 20) || (flags & ~1)) return PCAMV_EINVAL;
    int64_t nu = 0, ns = 0;
    pcamv_gpu_annexb_index(bytes, len, NULL, 0, &nu, &ns);
    pcamv_unit_t *units = (pcamv_unit_t *)malloc((size_t)(nu ? nu : 1) * sizeof(pcamv_unit_t));
    uint8_t *rbsp = (uint8_t *)malloc(len);
    struct Sl { size_t unit; int64_t start_bit, first_mb; } *sl = (Sl *)malloc((size_t)(nu ? nu : 1) * sizeof(Sl));
    int rc = units && rbsp && sl ? 0 : PCAMV_ENOMEM;
    int n = 0, qp = -1, id = -1, idc = -1;
    if (!rc) pcamv_gpu_annexb_index(bytes, len, units, (size_t)nu, &nu, &ns);
    /* the headers: every slice judged before any is decoded */
    for (int64_t k = 0; !rc && k < nu; k++) {
        const int type = units[k].nal_header < 0 ? 0 : units[k].nal_header & 31;
        if (type < 1 || type > 5) continue;
        if (type != 5) { rc = PCAMV_EUNSUP; break; }
        size_t rl = 0;
        rc = pcamv_gpu_nal_to_rbsp(bytes + units[k].off, (size_t)units[k].len, rbsp, &rl, NULL, NULL);
        if (rc) break;
        int32_t q = -1, pid = -1, dc = -1;
        Sl e = {(size_t)k, -1, -1};
        rc = pcamv_gpu_parse_idr_slice_header3(rbsp, rl, units[k].nal_header, params, &e.start_bit, &q, &pid, &dc, &e.first_mb);
        if (rc) break;
        if (n && (q != qp || pid != id || dc != idc)) { rc = PCAMV_EUNSUP; break; }
        if (e.first_mb % mb_w || e.first_mb >= (int64_t)mb_w * mb_h || (n ? e.first_mb <= sl[n - 1].first_mb : e.first_mb != 0)) { rc = PCAMV_EUNSUP; break; }
        qp = q; id = pid; idc = dc;
        sl[n++] = e;
    }
    if (!rc && !n) rc = PCAMV_EINVAL;
    if (!rc && n > 1 && idc == 2) rc = PCAMV_EUNSUP;
    const size_t lw = (size_t)16 * mb_w, cw = (size_t)8 * mb_w;
    for (int k = 0; !rc && k < n; k++) {
        const int r0 = (int)(sl[k].first_mb / mb_w), r1 = k + 1 < n ? (int)(sl[k + 1].first_mb / mb_w) : mb_h;
        size_t rl = 0;
        rc = pcamv_gpu_nal_to_rbsp(bytes + units[sl[k].unit].off, (size_t)units[sl[k].unit].len, rbsp, &rl, NULL, NULL);
        /* rows r0 .. r1 - 1 as a picture of their own: tightly packed planes of the same width are those rows of the picture's planes; a
         * slice that holds more or fewer macroblocks than its rows fails the decoder's end-of-slice rule, which is how overlap and gap show */
        if (!rc) rc = pcamv_gpu_decode_islice_cavlc2(rbsp, rl, (size_t)sl[k].start_bit, mb_w, r1 - r0, qp, chroma_qp_index_offset, flags,
                                                     y + (size_t)16 * r0 * lw, u + (size_t)8 * r0 * cw, v + (size_t)8 * r0 * cw);
        if (rc == PCAMV_EINVAL) rc = PCAMV_EUNSUP;             /* (the slices do not cover the picture as their first_mb says) */
    }
    if (!rc && idc != 1) rc = pcamv_gpu_deblock_intra_picture(y, u, v, mb_w, mb_h, qp, chroma_qp_index_offset);
    free(units); free(rbsp); free(sl);
    if (rc) return rc;
    *slice_qp = qp; *idr_pic_id = id; *n_slices = n;
    return 0;
}
extern "C" int pcamv_gpu_decode_idr_picture(const uint8_t *bytes, size_t len, int mb_w, int mb_h, const pcamv_stream_params_t *params, int chroma_qp_index_offset,
                                            uint8_t *y, uint8_t *u, uint8_t *v, int32_t *slice_qp, int32_t *idr_pic_id, int32_t *n_slices)
{
    return pcamv_gpu_decode_idr_picture2(bytes, len, mb_w, mb_h, params, chroma_qp_index_offset, 0, y, u, v, slice_qp, idr_pic_id, n_slices);
}
#endif
