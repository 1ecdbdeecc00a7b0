/*
 * pcamv_idr_i4x4.h -- Intra4x4 macroblocks beside Intra16x16 in the IDR picture the device codes: control code that compiles for the
 * device and for the host, behind pcamv_idr.h.
 *
 * On the device it is the body of k_idr_mb4 (pcamv_idr.hip); on the host it is what tests/fuzz/check_idr_i4x4.cpp compiles with the scalar
 * form of SP_LANES, to be decoded by pcamv_gpu_decode_islice_cavlc2 with its flag set (pcamv_mvsyntax.h), which stays the independent
 * check: the two share nothing but the code tables of sv_build_tables.  No HIP type.
 *
 * The rule (IdrPic::i4x4: 1 decide per macroblock, 2 every macroblock Intra4x4).  It is this coder's own and NOT the reference's, as
 * everything in pcamv_idr.h is.  idr_mb4 first codes the macroblock as idr_mb does -- the Intra16x16 choice, its reconstruction, counts
 * and bit string are idr_mb's, to the bit -- and keeps cost16, idr_mb's best_l (the SATD of the winning Intra16x16 mode, summed again from
 * what idr_mb left in its working memory).  Then the Intra4x4 trial, in the wave's working memory only: the sixteen blocks in
 * luma4x4BlkIdx order, each with the nine modes of 8.3.1.2 of which a mode is a candidate only if its neighbours exist (V, DDL, VL: the
 * row above; H, HU: the column to the left; DDR, VR, HD: both and the corner; DC always, in its four forms), available meaning in the
 * slice; the samples above-right come from the row above, for block 5 from the macroblock above-right ((mx + 1, my - 1): there iff the top
 * one is and mx + 1 < mb_w), and blocks 3, 7, 11, 13, 15 (and every block whose above-right samples are not there while the row above is)
 * take 8.3.1.2's substitution, the last sample above repeated; neighbours inside the macroblock are the trial's own reconstruction.
 * cost(m) = SATD4(src - pred_m) + lambda (m == predIntra4x4PredMode ? 1 : 4), the lowest wins, ties to the lower mode number;
 * predIntra4x4PredMode is 8.3.1.1's: the smaller of the modes of the blocks to the left and above, an Intra16x16 macroblock counting as
 * 2 (DC), and 2 when either block's macroblock is not available.  The chosen block is transformed (idr_fdct4), all sixteen coefficients
 * quantised by position class with idr_quant(.., dc = 0) -- the same dead zone and the same clamp to +-IDR_LEVEL_MAX --, dequantised as
 * the AC coefficients are, position 0 included (8.5.12.1 for a block that is no Intra16x16 one), idr_idct4, clip.
 * cost4 = IDR_I4_BIAS lambda + the sixteen winning costs; the macroblock becomes Intra4x4 iff cost4 < cost16 (i4x4 1) or always (2).
 * Only then its luma reconstruction, counts and bit string replace idr_mb's; chroma -- mode, levels, strings -- is idr_mb's either way.
 *
 * For the neighbours: nz gets total_coeff of the sixteen coefficients of each block (a block of an 8x8 whose pattern bit is 0 has no
 * level by construction, so its count is 0), and modes (IDR_MODE_BYTES a macroblock) the sixteen modes, or sixteen 2s.
 *
 * An Intra4x4 macroblock's bits (7.3.5, I slice): mb_type ue(0); sixteen times prev_intra4x4_pred_mode_flag [rem_intra4x4_pred_mode
 * u(3)]; intra_chroma_pred_mode ue; coded_block_pattern me(v) by the intra column of Table 9-4; mb_qp_delta se(0) only if the pattern is
 * not 0; of every 8x8 whose bit is set its four blocks of 16 (nC from the counts as above); chroma DC / AC as in idr_mb.  At most
 * IDR_MB_BITS_I4 bits (pcamv_idr_defs.h).
 *
 * Order between macroblocks: (x, y) reads (x - 1, y), (x, y - 1), (x - 1, y - 1) and (x + 1, y - 1): one launch per anti-diagonal
 * x + 2 y = d, the order of the loop filter.
 */
#ifndef PCAMV_IDR_I4X4_H
#define PCAMV_IDR_I4X4_H
#include "pcamv_idr.h"

struct IdrWork4 {
    uint8_t rec[256];                   /* the trial's reconstruction, 16 x 16 */
    uint8_t tr[4];                      /* the four samples above-right of block 5, from the macroblock above-right */
    uint8_t ml[4], mt[4];               /* the modes of the left macroblock's right column (by row) and of the top one's lowest row (by column) */
    uint8_t mode[16], cnt[16];
    int16_t lev[16][16];                /* all sixteen levels of a block in scan order */
    int cost[9];                        /* the block in hand: every candidate's cost, -1 for a mode that is none */
    int best[16], nclamp[16];
    uint32_t blk[16 * SWV_BLK_DWORDS], blen[16];
};

/* coded_block_pattern -> codeNum, the intra column of Table 9-4 (chroma_format_idc 1), indexed by cbp_luma | cbp_chroma << 4 */
SP_HD int idr_cbp_intra_code(int cbp)
{
    constexpr uint8_t t[48] = {3, 29, 30, 17, 31, 18, 37, 8, 32, 38, 19, 9, 20, 10, 11, 2,
                               16, 33, 34, 21, 35, 22, 39, 4, 36, 40, 23, 5, 24, 6, 7, 1,
                               41, 42, 43, 25, 44, 26, 46, 12, 45, 47, 27, 13, 28, 14, 15, 0};
    return t[cbp];
}
/* whether mode m of 8.3.1.2 may be used: avail bit 0 the column to the left, bit 1 the row above, bit 2 the corner */
SP_HD int idr_i4_mode_ok(int m, int avail)
{
    return m == 2 ? 1 : (m == 0 || m == 3 || m == 7) ? (avail >> 1) & 1 : (m == 1 || m == 8) ? avail & 1 : avail == 7;
}
/* 8.3.1.2.1 .. 8.3.1.2.9.  t[0] is p[-1, -1], t[1 + x] is p[x, -1] for x = 0 .. 7, l[y] is p[-1, y]; samples that are not there are never read
 * by a mode that idr_i4_mode_ok admits */
SP_HD void idr_i4_pred(const int t[9], const int l[4], int m, int avail, int out[16])
{
#define I4_T(i) t[1 + (i)]
#define I4_L(j) ((j) < 0 ? t[0] : l[j])
    if (m == 2) {
        const int st = I4_T(0) + I4_T(1) + I4_T(2) + I4_T(3), sl = l[0] + l[1] + l[2] + l[3];
        const int dc = (avail & 3) == 3 ? (st + sl + 4) >> 3 : (avail & 1) ? (sl + 2) >> 2 : (avail & 2) ? (st + 2) >> 2 : 128;
        for (int i = 0; i < 16; i++) out[i] = dc;
        return;
    }
    for (int i = 0; i < 16; i++) {
        const int x = i & 3, y = i >> 2;
        int v;
        if (m == 0) v = I4_T(x);
        else if (m == 1) v = l[y];
        else if (m == 3) v = x == 3 && y == 3 ? (I4_T(6) + 3 * I4_T(7) + 2) >> 2 : (I4_T(x + y) + 2 * I4_T(x + y + 1) + I4_T(x + y + 2) + 2) >> 2;
        else if (m == 4) v = x > y ? (I4_T(x - y - 2) + 2 * I4_T(x - y - 1) + I4_T(x - y) + 2) >> 2
                           : x < y ? (I4_L(y - x - 2) + 2 * I4_L(y - x - 1) + I4_L(y - x) + 2) >> 2 : (I4_T(0) + 2 * t[0] + l[0] + 2) >> 2;
        else if (m == 5) {
            const int z = 2 * x - y, k = x - (y >> 1);
            v = z >= 0 && !(z & 1) ? (I4_T(k - 1) + I4_T(k) + 1) >> 1 : z >= 0 ? (I4_T(k - 2) + 2 * I4_T(k - 1) + I4_T(k) + 2) >> 2
              : z == -1 ? (l[0] + 2 * t[0] + I4_T(0) + 2) >> 2 : (I4_L(y - 1) + 2 * I4_L(y - 2) + I4_L(y - 3) + 2) >> 2;
        } else if (m == 6) {
            const int z = 2 * y - x, k = y - (x >> 1);
            v = z >= 0 && !(z & 1) ? (I4_L(k - 1) + I4_L(k) + 1) >> 1 : z >= 0 ? (I4_L(k - 2) + 2 * I4_L(k - 1) + I4_L(k) + 2) >> 2
              : z == -1 ? (l[0] + 2 * t[0] + I4_T(0) + 2) >> 2 : (I4_T(x - 1) + 2 * I4_T(x - 2) + I4_T(x - 3) + 2) >> 2;
        } else if (m == 7) {
            const int k = x + (y >> 1);
            v = !(y & 1) ? (I4_T(k) + I4_T(k + 1) + 1) >> 1 : (I4_T(k) + 2 * I4_T(k + 1) + I4_T(k + 2) + 2) >> 2;
        } else {
            const int z = x + 2 * y, k = y + (x >> 1);
            v = z > 5 ? l[3] : z == 5 ? (l[2] + 3 * l[3] + 2) >> 2 : !(z & 1) ? (l[k] + l[k + 1] + 1) >> 1 : (l[k] + 2 * l[k + 1] + l[k + 2] + 2) >> 2;
        }
        out[i] = v;
    }
#undef I4_T
#undef I4_L
}

/* block b's neighbouring samples from the trial's reconstruction and the macroblock's edge (W.edge[0], as idr_mb loaded it); returns the
 * availability idr_i4_mode_ok and idr_i4_pred take.  mbavail: bit 0 left, bit 1 top, bit 2 the macroblock above-right */
SP_HD int idr_i4_gather(const IdrWork &W, const IdrWork4 &W4, int b, int mbavail, int t[9], int l[4])
{
    const int bx = idr_bx(b), by = idr_by(b), x0 = 4 * bx, y0 = 4 * by;
    const uint8_t *e = W.edge[0];
    const int left = bx > 0 || (mbavail & 1), top = by > 0 || (mbavail & 2);
    const int corner = bx > 0 && by > 0 ? 1 : bx > 0 ? (mbavail >> 1) & 1 : by > 0 ? mbavail & 1 : (mbavail & 3) == 3;
    /* above-right: inside the macroblock the block (bx + 1, by - 1) if it comes before this one, of the top row the macroblock above (block 5: above-right) */
    const int tr = by > 0 ? (bx < 3 && idr_blk_at(bx + 1, by - 1) < b) : bx < 3 ? (mbavail >> 1) & 1 : (mbavail >> 2) & 1;
    for (int k = 0; k < 9; k++) t[k] = 128;
    for (int k = 0; k < 4; k++) l[k] = 128;
    if (left) for (int k = 0; k < 4; k++) l[k] = bx > 0 ? W4.rec[16 * (y0 + k) + x0 - 1] : e[17 + y0 + k];
    if (top) {
        for (int k = 0; k < 4; k++) t[1 + k] = by > 0 ? W4.rec[16 * (y0 - 1) + x0 + k] : e[1 + x0 + k];
        for (int k = 4; k < 8; k++) t[1 + k] = !tr ? t[4] : by > 0 ? W4.rec[16 * (y0 - 1) + x0 + k] : bx < 3 ? e[1 + x0 + k] : W4.tr[k - 4];
    }
    if (corner) t[0] = bx > 0 && by > 0 ? W4.rec[16 * (y0 - 1) + x0 - 1] : bx > 0 ? e[x0] : by > 0 ? e[17 + y0 - 1] : e[0];
    return (left ? 1 : 0) | (top ? 2 : 0) | (corner ? 4 : 0);
}
/* 8.3.1.1 for block b: the smaller of the modes to the left and above; 2 when either block's macroblock is not available */
SP_HD int idr_i4_pred_mode(const IdrWork4 &W4, int b, int mbavail)
{
    const int bx = idr_bx(b), by = idr_by(b);
    const int a = bx > 0 ? W4.mode[idr_blk_at(bx - 1, by)] : (mbavail & 1) ? W4.ml[by] : -1;
    const int c = by > 0 ? W4.mode[idr_blk_at(bx, by - 1)] : (mbavail & 2) ? W4.mt[bx] : -1;
    return a < 0 || c < 0 ? 2 : a < c ? a : c;
}

/* ---------------------------------------------------------------- one macroblock, by one wavefront, with P.i4x4 != 0 */
PCAMV_DEV void idr_mb4(IdrWork &W, IdrWork4 &W4, const IdrPic &P, const uint16_t *vlc, int mx, int my)
{
    idr_mb(W, P, vlc, mx, my);                          /* the Intra16x16 macroblock, whole; ends with a barrier */
    if (!P.i4x4) return;                                /* (off: idr_mb, and P.modes is not there) */
    const int xy = my * P.mb_w + mx, lw = 16 * P.mb_w;
    const int top = my % idr_rows_per_slice(P.mb_h, P.slice_rows) > 0;
    const int mbavail = (mx > 0 ? 1 : 0) | (top ? 2 : 0) | (top && mx + 1 < P.mb_w ? 4 : 0), avail = mbavail & 3;
    /* what idr_mb decided, from what it left: the modes (its own loop) and cost16 */
    int mode_l = -1, mode_c = -1, cost16 = 0, best_c = 0;
    for (int m = 0; m < 4; m++) {
        int sl = 0, sc = 0;
        for (int b = 0; b < 16; b++) sl += (int)SP_UNI(W.satd[m][b]);
        for (int b = 16; b < 24; b++) sc += (int)SP_UNI(W.satd[m][b]);
        if ((int)SP_UNI(W.satd[m][0]) >= 0 && (mode_l < 0 || sl < cost16)) { mode_l = m; cost16 = sl; }
        if ((int)SP_UNI(W.satd[m][16]) >= 0 && (mode_c < 0 || sc < best_c)) { mode_c = m; best_c = sc; }
    }
    SP_LANES(l) {
        if (l < 4) {
            W4.tr[l] = (mbavail & 4) ? P.rec[0][(size_t)(16 * my - 1) * lw + 16 * (mx + 1) + l] : 128;
            W4.ml[l] = (mbavail & 1) ? P.modes[(size_t)(xy - 1) * IDR_MODE_BYTES + idr_blk_at(3, l)] : 2;
            W4.mt[l] = (mbavail & 2) ? P.modes[(size_t)(xy - P.mb_w) * IDR_MODE_BYTES + idr_blk_at(l, 3)] : 2;
        }
    }
    SP_SYNC();
    /* the trial: sixteen blocks one after the other; a lane per candidate mode, then the winner's lane codes the block */
    for (int b = 0; b < 16; b++) {
        const int x0 = 4 * idr_bx(b), y0 = 4 * idr_by(b), pm = idr_i4_pred_mode(W4, b, mbavail);
        SP_LANES(l) if (l < 9) {
            int t[9], e[4], p[16], d[16];
            const int av = idr_i4_gather(W, W4, b, mbavail, t, e);
            int c = -1;
            if (idr_i4_mode_ok(l, av)) {
                idr_i4_pred(t, e, l, av, p);
                for (int i = 0; i < 16; i++) d[i] = W.src[16 * (y0 + (i >> 2)) + x0 + (i & 3)] - p[i];
                c = idr_satd4(d) + P.lambda * (l == pm ? 1 : 4);
            }
            W4.cost[l] = c;
        }
        SP_SYNC();
        int win = 2, wc = (int)SP_UNI(W4.cost[2]);      /* DC is always a candidate */
        for (int m = 0; m < 9; m++) { const int c = (int)SP_UNI(W4.cost[m]); if (c >= 0 && (c < wc || (c == wc && m < win))) { win = m; wc = c; } }
        SP_LANES(l) if (l == win) {
            int t[9], e[4], p[16], d[16], c[16], r[16], nc = 0, cnt = 0;
            const int av = idr_i4_gather(W, W4, b, mbavail, t, e);
            idr_i4_pred(t, e, l, av, p);
            for (int i = 0; i < 16; i++) d[i] = W.src[16 * (y0 + (i >> 2)) + x0 + (i & 3)] - p[i];
            idr_fdct4(d, c);
            for (int i = 0; i < 16; i++) {
                const int pos = idr_zz(i), v = idr_quant(c[pos], P.qp, idr_cls(pos), P.dz, 0, &nc);
                W4.lev[b][i] = (int16_t)v; cnt += v != 0;
                d[pos] = v * idr_v(P.qp % 6, idr_cls(pos)) * (1 << (P.qp / 6));
            }
            idr_idct4(d, r);
            for (int i = 0; i < 16; i++) W4.rec[16 * (y0 + (i >> 2)) + x0 + (i & 3)] = (uint8_t)idr_clip8(p[i] + r[i]);
            W4.mode[b] = (uint8_t)l; W4.cnt[b] = (uint8_t)cnt; W4.best[b] = wc; W4.nclamp[b] = nc;
        }
        SP_SYNC();
    }
    int cost4 = IDR_I4_BIAS * P.lambda;
    for (int b = 0; b < 16; b++) cost4 += (int)SP_UNI(W4.best[b]);
    const int is4 = P.i4x4 == 2 || cost4 < cost16;
    if (!is4) {                                         /* stays Intra16x16: idr_mb's macroblock stands; the neighbours read sixteen DCs */
        SP_LANES(l) if (l < IDR_MODE_BYTES) P.modes[(size_t)xy * IDR_MODE_BYTES + l] = 2;
        SP_SYNC();
        return;
    }
    int cbp_l = 0, any_cac = 0, any_cdc = 0, nclamp = 0;
    for (int b = 0; b < 16; b++) { if ((int)SP_UNI(W4.cnt[b])) cbp_l |= 1 << (b >> 2); nclamp += (int)SP_UNI(W4.nclamp[b]); }
    for (int b = 16; b < 24; b++) { any_cac |= (int)SP_UNI(W.cnt[b]); nclamp += (int)SP_UNI(W.nclamp[b]); }
    for (int i = 0; i < 8; i++) any_cdc |= (int)SP_UNI(W.cdc[i >> 2][i & 3]) & 0xffff;
    nclamp += (int)SP_UNI(W.nclamp[25]) + (int)SP_UNI(W.nclamp[26]);
    const int cbp_c = any_cac ? 2 : any_cdc ? 1 : 0;
    /* the luma reconstruction, the counts and the modes go out; the sixteen blocks' bit strings, one lane per block */
    SP_LANES(l) {
        { const int y = l >> 2, x = 4 * (l & 3); for (int k = 0; k < 4; k++) P.rec[0][(size_t)(16 * my + y) * lw + 16 * mx + x + k] = W4.rec[16 * y + x + k]; }
        if (l < 16) {
            P.nz[(size_t)xy * IDR_NZ_BYTES + l] = W4.cnt[l];
            P.modes[(size_t)xy * IDR_MODE_BYTES + l] = W4.mode[l];
            const int x = idr_bx(l), y = idr_by(l);
            const int na = x > 0 ? W4.cnt[idr_blk_at(x - 1, y)] : (avail & 1) ? W.nzl[idr_blk_at(3, y)] : -1;
            const int nb = y > 0 ? W4.cnt[idr_blk_at(x, y - 1)] : (avail & 2) ? W.nzt[idr_blk_at(x, 3)] : -1;
            int bad = 0;
            const uint32_t e = swv_block(vlc, W4.blk + SWV_BLK_DWORDS * l, W4.lev[l], 16, idr_nc_class(na, nb), 1, bad);
            W4.blen[l] = bad || (e >> 16) ? 0x8000u : e;
        }
    }
    SP_SYNC();
    SP_LANES(l) if (l == 0) {
        uint32_t *slot = P.slots + (size_t)xy * IDR_SLOT_DWORDS;
        uint64_t acc = 0; int nb = 0, w = 0, bad = 0;
        auto put = [&](int nbits, uint32_t v) {           /* the low nbits <= 32 of v */
            if (nbits <= 0) return;
            acc = (acc << nbits) | (uint64_t)(nbits < 32 ? v & ((1u << nbits) - 1u) : v);
            nb += nbits;
            if (nb >= 32) { nb -= 32; if (w < IDR_SLOT_DWORDS) slot[w] = (uint32_t)(acc >> nb); else bad = 1; w++; }
        };
        auto ue = [&](uint32_t k) { const int len = 32 - __builtin_clz(k + 1u); put(len - 1, 0); put(len, k + 1u); };
        auto blockbits = [&](const uint32_t *blk, uint32_t e) {
            if (e & 0x8000u) { bad = 1; return; }
            const int bits = (int)(e & 0x7fffu);
            for (int k = 0; 32 * k < bits && k < SWV_BLK_DWORDS; k++) { const int nn = bits - 32 * k < 32 ? bits - 32 * k : 32; put(nn, blk[k] >> (32 - nn)); }
        };
        ue(0);                                          /* mb_type I_NxN */
        for (int b = 0; b < 16; b++) {
            const int pm = idr_i4_pred_mode(W4, b, mbavail), m = W4.mode[b];
            if (m == pm) put(1, 1); else put(4, (uint32_t)(m < pm ? m : m - 1));
        }
        ue((uint32_t)mode_c);
        ue((uint32_t)idr_cbp_intra_code(cbp_l | cbp_c << 4));
        if (cbp_l | cbp_c) put(1, 1);                   /* mb_qp_delta se(0) */
        for (int b = 0; b < 16; b++) if (cbp_l >> (b >> 2) & 1) blockbits(W4.blk + SWV_BLK_DWORDS * b, W4.blen[b]);
        if (cbp_c) { blockbits(W.blk + SWV_BLK_DWORDS * 25, W.blen[25]); blockbits(W.blk + SWV_BLK_DWORDS * 26, W.blen[26]); }
        if (cbp_c == 2) for (int b = 0; b < 8; b++) blockbits(W.blk + SWV_BLK_DWORDS * (17 + b), W.blen[17 + b]);
        const int total = 32 * w + nb;
        if (nb) { if (w < IDR_SLOT_DWORDS) slot[w] = (uint32_t)(acc << (32 - nb)); else bad = 1; }
        P.bits[xy] = bad || total > IDR_MB_BITS_I4 ? -1 : total;
        if (P.clamped) P.clamped[xy] = nclamp;
    }
    SP_SYNC();
}
#endif
