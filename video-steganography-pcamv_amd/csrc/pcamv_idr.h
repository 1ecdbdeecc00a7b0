/*
 * pcamv_idr.h -- the IDR picture a chain starts with, coded on the device: control code that compiles for the device and for the host.
 *
 * On the device it is the body of k_idr_mb, k_idr_prefix, k_idr_pack and k_idr_unit and of their siblings for pictures of several slices
 * (pcamv_idr.hip); on the host it is what tests/fuzz/check_idr_write.cpp and check_idr_slices.cpp compile with the scalar form of
 * SP_LANES (pcamv_slice_parse.h), to be decoded by the library's host decoder pcamv_gpu_decode_islice_cavlc (pcamv_mvsyntax.h), which stays the independent check: the two share nothing but the code
 * tables of sv_build_tables.  No HIP type.  Included behind pcamv_slice_write_cavlc.h (swv_block: a residual block's bit string by one
 * lane; the output path behind a final byte) and pcamv_stream_write.h (the bit writer of the slice headers).
 *
 * Scope, fixed: one I slice per picture, or several of whole macroblock rows (IdrPic::slice_rows; the layout: pcamv_idr_defs.h),
 * Intra16x16 macroblocks -- behind a flag Intra4x4 ones beside them (IdrPic::i4x4: idr_mb4 of pcamv_idr_i4x4.h, which begins with
 * idr_mb and replaces its luma where the Intra4x4 trial costs less; with the flag at 0 nothing here is touched) -- (luma V / H / DC / plane, chroma DC / H / V / plane, each chosen by
 * SATD among the modes whose neighbours exist, ties to the lower mode number of 8.3.3 / 8.3.4), one QP (mb_qp_delta 0), CAVLC whatever
 * the stream's P slices use, disable_deblocking_filter_idc 1: the reconstruction a decoder makes is the unfiltered one that is made here
 * and becomes the chain's reference (or, where the caller asks for a filtered picture, goes through pcamv_idr_deblock.h first, behind
 * the whole picture's coding: nothing here changes with that, intra prediction reads unfiltered samples).  This is NOT the reference's I-frame coder (its own I4x4 rule, no RD decision, its own mode order): an I
 * picture carries no payload, and the P chain's exactness is defined given its reference picture.
 *
 * Arithmetic.  Forward: the core transform of 8.5 backwards on the 4x4 residuals; the sixteen luma DCs through a 4x4 Hadamard with
 * (x + 1) >> 1, the four DCs of a chroma plane through a 2x2 one.  Quantiser: |level| = (|c| * MF + f) >> (15 + qp / 6) with the flat
 * matrices' MF (13107 5243 8066 / ... by qp % 6 and position class) and f = deadzone << (9 + qp / 6), deadzone = i_luma_deadzone[1] of
 * 64; a DC takes MF of class 0, one more bit of shift and 2 f.  Every level is then clamped to +-IDR_LEVEL_MAX (derived below) BEFORE
 * reconstruction, which is 8.5.10 / 8.5.11 / 8.5.12 on the clamped levels in 32-bit integers: what the decoder does.
 *
 * The level bound.  CAVLC below the High profiles has no level_prefix above 15 (9.2.2.1).  A level behind suffixLength s is coded as
 * levelCode = 2 |v| - 2 + (v < 0); prefix 15 carries levelCode - (15 << s) (and - 15 more at s = 0) in a suffix of 12 bits, so at most
 * 4095.  levelCode <= 4095 + 30 at s = 0 and s = 1 -- the tightest of the seven suffix lengths, 15 << s growing with s -- gives
 * 2 |v| - 1 <= 4125, |v| <= 2063.  (The first level behind fewer than three trailing ones is coded one nearer to zero, which only
 * helps.)  swv_level's own clip (pcamv_slice_write_cavlc.h) is therefore never reached from here: check_idr_write.cpp requires it.
 *
 * One macroblock's bits (7.3.5 for an I slice): mb_type ue(1 + mode + 4 cbp_chroma + 12 (cbp_luma == 15)), intra_chroma_pred_mode ue,
 * mb_qp_delta se(0), Intra16x16DCLevel (always; nC as for luma block 0), the sixteen Intra16x16ACLevel blocks of 15 if any of them
 * has a level (cbp_luma 15, else 0), chroma DC if any chroma level, chroma AC if any chroma AC level.  total_coeff of the AC blocks is
 * what neighbours read for nC (9.2.1); availability is the slice's edge: the picture's, or with slice_rows the first row of the slice.
 * CAVLC in an I slice has no
 * serial state -- no skip run, a constant QP -- so every macroblock's bit string is made where the macroblock is coded, into its own
 * slot of IDR_SLOT_DWORDS, and a prefix over the lengths places them.
 *
 * Memory per context (IdrPic): 24 counts, a slot and a length per macroblock, a prefix entry per macroblock, the RBSP; with i4x4 the
 * sixteen Intra4x4PredModes of every macroblock.
 */
#ifndef PCAMV_IDR_H
#define PCAMV_IDR_H
#include "pcamv_slice_write_cavlc.h"
#include "pcamv_idr_defs.h"

struct IdrWork {
    uint8_t src[384], pred[384];        /* Y 16 x 16, U 8 x 8, V 8 x 8 */
    uint8_t edge[3][36];                /* per plane: [0] above-left, [1 .. 16] the line above, [17 .. 32] the column to the left (chroma: 8 of each) */
    int satd[4][24];                    /* [mode][block] */
    int16_t lev[24][16];                /* a block's levels in scan order; [0] stays 0 (the DC goes its own way) */
    int16_t dcl[16], cdc[2][4];         /* the DC levels in scan order */
    int dcw[24];                        /* a block's DC: the transform's, then the dequantised one */
    uint8_t cnt[IDR_NZ_BYTES], nzl[IDR_NZ_BYTES], nzt[IDR_NZ_BYTES];
    uint32_t blk[IDR_NBLK * SWV_BLK_DWORDS], blen[IDR_NBLK];
    int nclamp[24 + 3];
};

SP_HD int idr_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
SP_HD int idr_zz(int i) { return (int)((0xFEB7ADC963258410ull >> (4 * i)) & 15u); }      /* the frame scan: 0 1 4 8 5 2 3 6 9 12 13 10 7 11 14 15 */
SP_HD int idr_bx(int b) { return (b & 1) | ((b >> 1) & 2); }
SP_HD int idr_by(int b) { return ((b >> 1) & 1) | ((b >> 2) & 2); }
SP_HD int idr_blk_at(int x, int y) { return (x & 1) | (y & 1) << 1 | (x & 2) << 1 | (y & 2) << 2; }
SP_HD int idr_cls(int pos) { const int i = pos >> 2, j = pos & 3; return !(i & 1) && !(j & 1) ? 0 : (i & 1) && (j & 1) ? 1 : 2; }
SP_HD int idr_mf(int q6, int cls)
{
    const int t = cls == 0 ? (q6 == 0 ? 13107 : q6 == 1 ? 11916 : q6 == 2 ? 10082 : q6 == 3 ? 9362 : q6 == 4 ? 8192 : 7282)
                : cls == 1 ? (q6 == 0 ? 5243 : q6 == 1 ? 4660 : q6 == 2 ? 4194 : q6 == 3 ? 3647 : q6 == 4 ? 3355 : 2893)
                           : (q6 == 0 ? 8066 : q6 == 1 ? 7490 : q6 == 2 ? 6554 : q6 == 3 ? 5825 : q6 == 4 ? 5243 : 4559);
    return t;
}
SP_HD int idr_v(int q6, int cls)
{
    return cls == 0 ? (q6 == 0 ? 10 : q6 == 1 ? 11 : q6 == 2 ? 13 : q6 == 3 ? 14 : q6 == 4 ? 16 : 18)
         : cls == 1 ? (q6 == 0 ? 16 : q6 == 1 ? 18 : q6 == 2 ? 20 : q6 == 3 ? 23 : q6 == 4 ? 25 : 29)
                    : (q6 == 0 ? 13 : q6 == 1 ? 14 : q6 == 2 ? 16 : q6 == 3 ? 18 : q6 == 4 ? 20 : 23);
}
/* |c| quantised at qp (dc: one more bit, twice the rounding), signed, clamped; *nclamp counts the clamped ones */
SP_HD int idr_quant(int c, int qp, int cls, int dz, int dc, int *nclamp)
{
    const int qbits = 15 + qp / 6 + dc;
    const long long f = (long long)dz << (qbits - 6);
    long long a = ((long long)(c < 0 ? -c : c) * idr_mf(qp % 6, cls) + f) >> qbits;
    if (a > IDR_LEVEL_MAX) { a = IDR_LEVEL_MAX; (*nclamp)++; }
    return c < 0 ? -(int)a : (int)a;
}
/* 8.5.10's matrix (1 1 1 1 / 1 1 -1 -1 / 1 -1 -1 1 / 1 -1 1 -1) on both sides of a 4 x 4 block, no scaling: symmetric, its own inverse up to 16 */
SP_HD void idr_hadamard4(const int *in, int *out)
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int a = in[4 * i] + in[4 * i + 1], b = in[4 * i] - in[4 * i + 1], c = in[4 * i + 2] + in[4 * i + 3], d = in[4 * i + 2] - in[4 * i + 3];
        t[4 * i] = a + c; t[4 * i + 1] = a - c; t[4 * i + 2] = b - d; t[4 * i + 3] = b + d;
    }
    for (int j = 0; j < 4; j++) {
        const int a = t[j] + t[4 + j], b = t[j] - t[4 + j], c = t[8 + j] + t[12 + j], d = t[8 + j] - t[12 + j];
        out[j] = a + c; out[4 + j] = a - c; out[8 + j] = b - d; out[12 + j] = b + d;
    }
}

/* the plane parameters (8.3.3.4, 8.3.4.4) of an edge: n = 16 (luma) or 8 (chroma) */
SP_HD void idr_plane_abc(const uint8_t *e, int n, int *a, int *b, int *c)
{
    const int h = n / 2;
    int H = 0, V = 0;
    for (int k = 0; k < h; k++) {
        const int hi = h + k, lo = h - 2 - k;           /* lo = -1: the sample above-left */
        H += (k + 1) * (e[1 + hi] - (lo < 0 ? e[0] : e[1 + lo]));
        V += (k + 1) * (e[17 + hi] - (lo < 0 ? e[0] : e[17 + lo]));
    }
    *a = 16 * (e[17 + n - 1] + e[1 + n - 1]);
    *b = n == 16 ? (5 * H + 32) >> 6 : (34 * H + 32) >> 6;
    *c = n == 16 ? (5 * V + 32) >> 6 : (34 * V + 32) >> 6;
}
/* the prediction of the 4x4 block at (x0, y0) of a plane of n x n: mode in the plane's own numbering (luma 0 V 1 H 2 DC 3 plane; chroma
 * 0 DC 1 H 2 V 3 plane), avail bit 0 left, bit 1 top */
SP_HD void idr_pred4(const uint8_t *e, int n, int luma, int mode, int avail, int x0, int y0, int out[16])
{
    const int kind = luma ? (mode == 0 ? 2 : mode == 1 ? 1 : mode == 2 ? 0 : 3) : mode;        /* 0 DC 1 H 2 V 3 plane */
    if (kind == 1) { for (int i = 0; i < 16; i++) out[i] = e[17 + y0 + (i >> 2)]; return; }
    if (kind == 2) { for (int i = 0; i < 16; i++) out[i] = e[1 + x0 + (i & 3)]; return; }
    if (kind == 3) {
        int a, b, c;
        idr_plane_abc(e, n, &a, &b, &c);
        const int o = n / 2 - 1;
        for (int i = 0; i < 16; i++) out[i] = idr_clip8((a + b * (x0 + (i & 3) - o) + c * (y0 + (i >> 2) - o) + 16) >> 5);
        return;
    }
    int dc = 128;
    if (luma) {
        int st = 0, sl = 0;
        for (int k = 0; k < 16; k++) { st += e[1 + k]; sl += e[17 + k]; }
        dc = avail == 3 ? (st + sl + 16) >> 5 : avail == 2 ? (st + 8) >> 4 : avail == 1 ? (sl + 8) >> 4 : 128;
    } else {
        int st = 0, sl = 0;
        for (int k = 0; k < 4; k++) { st += e[1 + x0 + k]; sl += e[17 + y0 + k]; }
        const int top = avail & 2, left = avail & 1;
        if (x0 == y0) dc = top && left ? (st + sl + 4) >> 3 : top ? (st + 2) >> 2 : left ? (sl + 2) >> 2 : 128;
        else if (x0) dc = top ? (st + 2) >> 2 : left ? (sl + 2) >> 2 : 128;
        else dc = left ? (sl + 2) >> 2 : top ? (st + 2) >> 2 : 128;
    }
    for (int i = 0; i < 16; i++) out[i] = dc;
}
SP_HD int idr_satd4(const int d[16])
{
    int t[16], s = 0;
    idr_hadamard4(d, t);
    for (int i = 0; i < 16; i++) s += t[i] < 0 ? -t[i] : t[i];
    return s;
}
/* the core transform of a 4x4 residual (the inverse of 8.5.12's, unscaled) */
SP_HD void idr_fdct4(const int d[16], int out[16])
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int s03 = d[4 * i] + d[4 * i + 3], d03 = d[4 * i] - d[4 * i + 3], s12 = d[4 * i + 1] + d[4 * i + 2], d12 = d[4 * i + 1] - d[4 * i + 2];
        t[4 * i] = s03 + s12; t[4 * i + 1] = 2 * d03 + d12; t[4 * i + 2] = s03 - s12; t[4 * i + 3] = d03 - 2 * d12;
    }
    for (int j = 0; j < 4; j++) {
        const int s03 = t[j] + t[12 + j], d03 = t[j] - t[12 + j], s12 = t[4 + j] + t[8 + j], d12 = t[4 + j] - t[8 + j];
        out[j] = s03 + s12; out[4 + j] = 2 * d03 + d12; out[8 + j] = s03 - s12; out[12 + j] = d03 - 2 * d12;
    }
}
/* 8.5.12: the residual of dequantised coefficients, rounded */
SP_HD void idr_idct4(const int d[16], int out[16])
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int e0 = d[4 * i] + d[4 * i + 2], e1 = d[4 * i] - d[4 * i + 2], e2 = (d[4 * i + 1] >> 1) - d[4 * i + 3], e3 = d[4 * i + 1] + (d[4 * i + 3] >> 1);
        t[4 * i] = e0 + e3; t[4 * i + 1] = e1 + e2; t[4 * i + 2] = e1 - e2; t[4 * i + 3] = e0 - e3;
    }
    for (int j = 0; j < 4; j++) {
        const int e0 = t[j] + t[8 + j], e1 = t[j] - t[8 + j], e2 = (t[4 + j] >> 1) - t[12 + j], e3 = t[4 + j] + (t[12 + j] >> 1);
        out[j] = (e0 + e3 + 32) >> 6; out[4 + j] = (e1 + e2 + 32) >> 6; out[8 + j] = (e1 - e2 + 32) >> 6; out[12 + j] = (e0 - e3 + 32) >> 6;
    }
}
/* the coeff_token class of a block from the counts of its left and upper neighbours (9.2.1); a negative count: not available */
SP_HD int idr_nc_class(int na, int nb)
{
    const int nc = na >= 0 && nb >= 0 ? (na + nb + 1) >> 1 : na >= 0 ? na : nb >= 0 ? nb : 0;
    return nc < 2 ? 0 : nc < 4 ? 1 : nc < 8 ? 2 : 3;
}

/* block l of the macroblock (0..15 luma by luma4x4BlkIdx, 16..19 Cb, 20..23 Cr in raster order): plane, edge length, place */
#define IDR_BLOCK_GEOM(l) \
    const int pl = (l) < 16 ? 0 : (l) < 20 ? 1 : 2, n = pl ? 8 : 16, \
              x0 = pl ? 4 * (((l) - 16) & 1) : 4 * idr_bx(l), y0 = pl ? 4 * ((((l) - 16) >> 1) & 1) : 4 * idr_by(l), \
              sbase = pl == 0 ? 0 : pl == 1 ? 256 : 320

/* ---------------------------------------------------------------- one macroblock, by one wavefront */
/* Reads the source block and, from rec, the unfiltered neighbours (left, top, top-left) and their counts: the macroblocks of the
 * anti-diagonals before this one's are done.  Writes the block's reconstruction, counts, bit string and bit count. */
PCAMV_DEV void idr_mb(IdrWork &W, const IdrPic &P, const uint16_t *vlc, int mx, int my)
{
    /* available means in the slice (P.slice_rows whole rows): left always is, top and top-left are below the slice's first row */
    const int xy = my * P.mb_w + mx, avail = (mx > 0 ? 1 : 0) | (my % idr_rows_per_slice(P.mb_h, P.slice_rows) > 0 ? 2 : 0);
    const int lw = 16 * P.mb_w, cw = 8 * P.mb_w;
    SP_SYNC();
    SP_LANES(l) {
        /* source: a lane takes four luma pixels, the first 32 lanes four chroma pixels */
        { const int y = l >> 2, x = 4 * (l & 3); for (int k = 0; k < 4; k++) W.src[16 * y + x + k] = P.src[0][(size_t)(16 * my + y) * lw + 16 * mx + x + k]; }
        if (l < 32) { const int c = l >> 4, y = (l & 15) >> 1, x = 4 * (l & 1); for (int k = 0; k < 4; k++) W.src[256 + 64 * c + 8 * y + x + k] = P.src[1 + c][(size_t)(8 * my + y) * cw + 8 * mx + x + k]; }
        /* edges: lanes 0..32 luma, 33..49 Cb, 50..63 + ... : one sample each, by a flat index over the three planes' 33 + 17 + 17 */
        for (int q = l; q < 67; q += 64) {
            const int c = q < 33 ? 0 : q < 50 ? 1 : 2, k = q - (c == 0 ? 0 : c == 1 ? 33 : 50), nn = c ? 8 : 16, w = c ? cw : lw, px = nn * mx, py = nn * my;
            const uint8_t *r = P.rec[c];
            int v = 128, at = 0;
            if (k == 0) { at = 0; if (avail == 3) v = r[(size_t)(py - 1) * w + px - 1]; }
            else if (k <= nn) { at = k; if (avail & 2) v = r[(size_t)(py - 1) * w + px + k - 1]; }
            else { at = 17 + (k - nn - 1); if (avail & 1) v = r[(size_t)(py + k - nn - 1) * w + px - 1]; }
            W.edge[c][at] = (uint8_t)v;
        }
        if (l < IDR_NZ_BYTES) {
            W.nzl[l] = mx > 0 ? P.nz[(size_t)(xy - 1) * IDR_NZ_BYTES + l] : 0;
            W.nzt[l] = (avail & 2) ? P.nz[(size_t)(xy - P.mb_w) * IDR_NZ_BYTES + l] : 0;
        }
        if (l < 27) W.nclamp[l] = 0;
    }
    SP_SYNC();
    /* every block's SATD under every mode its plane may use */
    SP_LANES(l) if (l < 24) {
        IDR_BLOCK_GEOM(l);
        for (int m = 0; m < 4; m++) {
            const int kind = pl ? m : (m == 0 ? 2 : m == 1 ? 1 : m == 2 ? 0 : 3);
            const bool ok = kind == 0 || (kind == 1 && (avail & 1)) || (kind == 2 && (avail & 2)) || (kind == 3 && avail == 3);
            int s = 0;
            if (ok) {
                int p[16], d[16];
                idr_pred4(W.edge[pl], n, !pl, m, avail, x0, y0, p);
                for (int i = 0; i < 16; i++) d[i] = W.src[sbase + n * (y0 + (i >> 2)) + x0 + (i & 3)] - p[i];
                s = idr_satd4(d);
            }
            W.satd[m][l] = ok ? s : -1;
        }
    }
    SP_SYNC();
    int mode_l = -1, mode_c = -1, best_l = 0, best_c = 0;
    for (int m = 0; m < 4; m++) {
        int sl = 0, sc = 0;
        for (int b = 0; b < 16; b++) sl += (int)SP_UNI(W.satd[m][b]);
        for (int b = 16; b < 24; b++) sc += (int)SP_UNI(W.satd[m][b]);
        if ((int)SP_UNI(W.satd[m][0]) >= 0 && (mode_l < 0 || sl < best_l)) { mode_l = m; best_l = sl; }
        if ((int)SP_UNI(W.satd[m][16]) >= 0 && (mode_c < 0 || sc < best_c)) { mode_c = m; best_c = sc; }
    }
    /* prediction, transform, the AC levels */
    SP_LANES(l) if (l < 24) {
        IDR_BLOCK_GEOM(l);
        int p[16], d[16], c[16], nc = 0;
        idr_pred4(W.edge[pl], n, !pl, pl ? mode_c : mode_l, avail, x0, y0, p);
        for (int i = 0; i < 16; i++) { W.pred[sbase + n * (y0 + (i >> 2)) + x0 + (i & 3)] = (uint8_t)p[i]; d[i] = W.src[sbase + n * (y0 + (i >> 2)) + x0 + (i & 3)] - p[i]; }
        idr_fdct4(d, c);
        W.dcw[l] = c[0];
        W.lev[l][0] = 0;
        for (int i = 1; i < 16; i++) { const int pos = idr_zz(i); W.lev[l][i] = (int16_t)idr_quant(c[pos], pl ? P.qpc : P.qp, idr_cls(pos), P.dz, 0, &nc); }
        W.nclamp[l] = nc;
    }
    SP_SYNC();
    /* the DC levels and the dequantised DCs: lane 0 luma (8.5.10), lanes 1 / 2 a chroma plane each (8.5.11) */
    SP_LANES(l) if (l < 3) {
        int nc = 0;
        if (l == 0) {
            int m[16], h[16], lv[16], f[16];
            for (int b = 0; b < 16; b++) m[4 * idr_by(b) + idr_bx(b)] = W.dcw[b];
            idr_hadamard4(m, h);
            for (int i = 0; i < 16; i++) lv[i] = idr_quant((h[i] + 1) >> 1, P.qp, 0, P.dz, 1, &nc);
            for (int i = 0; i < 16; i++) W.dcl[i] = (int16_t)lv[idr_zz(i)];
            idr_hadamard4(lv, f);
            const int v0 = idr_v(P.qp % 6, 0), q = P.qp / 6;
            for (int b = 0; b < 16; b++) {
                const int fv = f[4 * idr_by(b) + idr_bx(b)];
                W.dcw[b] = q >= 2 ? fv * v0 * (1 << (q - 2)) : (fv * v0 + (1 << (1 - q))) >> (2 - q);
            }
        } else {
            const int c0 = 16 + 4 * (l - 1);
            const int a = W.dcw[c0], b = W.dcw[c0 + 1], c = W.dcw[c0 + 2], d = W.dcw[c0 + 3];
            const int h[4] = {a + b + c + d, a - b + c - d, a + b - c - d, a - b - c + d};
            int lv[4];
            for (int i = 0; i < 4; i++) { lv[i] = idr_quant(h[i], P.qpc, 0, P.dz, 1, &nc); W.cdc[l - 1][i] = (int16_t)lv[i]; }
            const int f[4] = {lv[0] + lv[1] + lv[2] + lv[3], lv[0] - lv[1] + lv[2] - lv[3], lv[0] + lv[1] - lv[2] - lv[3], lv[0] - lv[1] - lv[2] + lv[3]};
            const int v0 = idr_v(P.qpc % 6, 0), q = P.qpc / 6;
            for (int i = 0; i < 4; i++) W.dcw[c0 + i] = (f[i] * 16 * v0 * (1 << q)) >> 5;
        }
        W.nclamp[24 + l] = nc;
    }
    SP_SYNC();
    /* reconstruction and the counts */
    SP_LANES(l) if (l < 24) {
        IDR_BLOCK_GEOM(l);
        const int qp = pl ? P.qpc : P.qp;
        int d[16], r[16], cnt = 0;
        d[0] = W.dcw[l];
        for (int i = 1; i < 16; i++) { const int pos = idr_zz(i), v = W.lev[l][i]; cnt += v != 0; d[pos] = v * idr_v(qp % 6, idr_cls(pos)) * (1 << (qp / 6)); }
        idr_idct4(d, r);
        W.cnt[l] = (uint8_t)cnt;
        uint8_t *dst = P.rec[pl] + (size_t)(n * my + y0) * (pl ? cw : lw) + n * mx + x0;
        for (int i = 0; i < 16; i++) dst[(size_t)(i >> 2) * (pl ? cw : lw) + (i & 3)] = (uint8_t)idr_clip8(W.pred[sbase + n * (y0 + (i >> 2)) + x0 + (i & 3)] + r[i]);
    }
    SP_SYNC();
    int any_l = 0, any_cac = 0, any_cdc = 0, nclamp = 0;
    for (int b = 0; b < 16; b++) any_l |= (int)SP_UNI(W.cnt[b]);
    for (int b = 16; b < 24; b++) any_cac |= (int)SP_UNI(W.cnt[b]);
    for (int i = 0; i < 8; i++) any_cdc |= (int)SP_UNI(W.cdc[i >> 2][i & 3]) & 0xffff;
    for (int i = 0; i < 27; i++) nclamp += (int)SP_UNI(W.nclamp[i]);
    const int cbp_c = any_cac ? 2 : any_cdc ? 1 : 0;
    /* every block's bit string, one lane per block (swv_block); the counts go out for the macroblocks to the right and below */
    SP_LANES(l) {
        if (l < IDR_NZ_BYTES) P.nz[(size_t)xy * IDR_NZ_BYTES + l] = W.cnt[l];
        if (l < IDR_NBLK) {
            const int16_t *lv = l == 0 ? W.dcl : l <= 24 ? W.lev[l - 1] + 1 : W.cdc[l - 25];
            const int count = l == 0 ? 16 : l <= 24 ? 15 : 4;
            int tab = 4;
            if (l <= 24) {
                const int b = l == 0 ? 0 : l - 1;
                int na, nb;
                if (b < 16) {
                    const int x = idr_bx(b), y = idr_by(b);
                    na = x > 0 ? W.cnt[idr_blk_at(x - 1, y)] : (avail & 1) ? W.nzl[idr_blk_at(3, y)] : -1;
                    nb = y > 0 ? W.cnt[idr_blk_at(x, y - 1)] : (avail & 2) ? W.nzt[idr_blk_at(x, 3)] : -1;
                } else {
                    const int base = b < 20 ? 16 : 20, x = (b - base) & 1, y = (b - base) >> 1;
                    na = x > 0 ? W.cnt[base + 2 * y] : (avail & 1) ? W.nzl[base + 2 * y + 1] : -1;
                    nb = y > 0 ? W.cnt[base + x] : (avail & 2) ? W.nzt[base + 2 + x] : -1;
                }
                tab = idr_nc_class(na, nb);
            }
            int bad = 0;
            const uint32_t e = swv_block(vlc, W.blk + SWV_BLK_DWORDS * l, lv, count, tab, 1, bad);
            W.blen[l] = bad || (e >> 16) ? 0x8000u : e;          /* a string too long, or a level the clamp should have kept from swv_level's clip */
        }
    }
    SP_SYNC();
    /* the macroblock's bits, by one lane: mb_type, intra_chroma_pred_mode, mb_qp_delta, the blocks the pattern codes in syntax order */
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
        auto blockbits = [&](int id) {
            const uint32_t e = W.blen[id];
            if (e & 0x8000u) { bad = 1; return; }
            const int bits = (int)(e & 0x7fffu);
            for (int k = 0; 32 * k < bits && k < SWV_BLK_DWORDS; k++) { const int nn = bits - 32 * k < 32 ? bits - 32 * k : 32; put(nn, W.blk[SWV_BLK_DWORDS * id + k] >> (32 - nn)); }
        };
        ue((uint32_t)(1 + mode_l + 4 * cbp_c + (any_l ? 12 : 0)));
        ue((uint32_t)mode_c);
        put(1, 1);
        blockbits(0);
        if (any_l) for (int b = 0; b < 16; b++) blockbits(1 + b);
        if (cbp_c) { blockbits(25); blockbits(26); }
        if (cbp_c == 2) for (int b = 0; b < 8; b++) blockbits(17 + b);
        const int total = 32 * w + nb;
        if (nb) { if (w < IDR_SLOT_DWORDS) slot[w] = (uint32_t)(acc << (32 - nb)); else bad = 1; }
        P.bits[xy] = bad || total > IDR_MB_BITS ? -1 : total;
        if (P.clamped) P.clamped[xy] = nclamp;
    }
    SP_SYNC();
}

/* ---------------------------------------------------------------- the RBSP: one destination dword */
/* pre[0 .. n_mb]: the bit at which each macroblock's string begins (pre[0] = the header's bits), pre[n_mb] = the bit of the stop bit.
 * Dword k of the RBSP -- bits 32 k .. 32 k + 31, the first in bit 31 -- from the header, the macroblocks that reach into it (found by a
 * search in the prefix) and rbsp_trailing_bits; stored so that its bytes are in stream order.  This is the merge a writer of per-block
 * or per-macroblock strings needs: nothing in it knows what the strings hold. */
SP_HD uint32_t idr_take(const uint32_t *s, long long from, int nbits)       /* bits from .. from + nbits - 1 (nbits <= 32) of a string of dwords */
{
    const long long d = from >> 5; const int sh = (int)(from & 31);
    const uint64_t two = (uint64_t)s[d] << 32 | (sh + nbits > 32 ? s[d + 1] : 0u);
    return (uint32_t)((two << sh) >> 32) >> (32 - nbits);
}
SP_HD uint32_t idr_pack_dword(long long k, const uint8_t *hdr, int hdr_bits, const long long *pre, const uint32_t *slots, int n_mb)
{
    const long long lo = 32 * k, hi = lo + 32, end = pre[n_mb];
    uint32_t out = 0;
    for (long long b = lo; b < hi && b < hdr_bits; b++) out |= (uint32_t)((hdr[b >> 3] >> (7 - (b & 7))) & 1) << (31 - (int)(b - lo));
    /* the last macroblock that begins at or before lo */
    int a = 0, z = n_mb;
    while (z - a > 1) { const int m = (a + z) >> 1; if (pre[m] <= lo) a = m; else z = m; }
    for (int i = a; i < n_mb && pre[i] < hi; i++) {
        const long long s0 = pre[i] > lo ? pre[i] : lo, s1 = pre[i + 1] < hi ? pre[i + 1] : hi;
        if (s1 <= s0) continue;
        const int nbits = (int)(s1 - s0);
        out |= idr_take(slots + (size_t)i * IDR_SLOT_DWORDS, s0 - pre[i], nbits) << (32 - nbits) >> (int)(s0 - lo);
    }
    if (end >= lo && end < hi) out |= 1u << (31 - (int)(end - lo));                 /* rbsp_stop_one_bit; the alignment zeros are there */
    return __builtin_bswap32(out);
}

/* ---------------------------------------------------------------- the unit: what the slice writers' as_nal path does, on a finished RBSP */
struct IdrOut {                         /* the members sw_emit works on (pcamv_slice_write_common.h) */
    uint8_t *dst; long long cap, n;
    uint32_t *obuf; int fill;
    long long abase;
    int as_nal, zeros;
};
/* rbsp[0, len) into dst[0, cap): (as_nal) long start code, header byte, emulation prevention.  win: 64 dwords.  Returns 0 and *len_out, or
 * PCAMV_ENOMEM with *len_out = 0; nothing is stored at or beyond cap */
/* The walk itself.  count != 0: the length pass of a picture of several slices -- the same walk with no room at all (sw_raw counts what it
 * does not store), carried to the end whatever the count: returns 0 and the unit's length, nothing stored */
PCAMV_DEV int idr_unit_walk(IdrOut &O, uint32_t *win, const uint8_t *rbsp, long long len, int nal_byte, int as_nal, uint8_t *dst, long long cap, int count, long long *len_out)
{
    *len_out = 0;
    if (count) cap = 0;
    sw_out_begin(O, dst, cap);
    if (as_nal) { sw_raw(O, 0); sw_raw(O, 0); sw_raw(O, 0); sw_raw(O, 1); sw_raw(O, (uint32_t)nal_byte & 255u); O.as_nal = 1; }
    for (long long base = 0; base < len; base += 256) {             /* rbsp is dword-aligned and padded to whole dwords */
        SP_SYNC();
        SP_LANES(l) win[l] = base + 4 * l < len ? sp_ld32(rbsp + base + 4 * l) : 0u;
        SP_SYNC();
        const int m = len - base < 256 ? (int)(len - base) : 256;
        for (int k = 0; k < m; k++) sw_emit(O, SP_UNI(win[k >> 2]) >> (8 * (k & 3)));
        if (!count && O.n > O.cap) return PCAMV_ENOMEM;
    }
    if (count) { *len_out = O.n; return 0; }
    if (O.n > O.cap) return PCAMV_ENOMEM;
    if (O.fill) sw_flush(O);
    *len_out = O.n;
    return 0;
}
PCAMV_DEV int idr_unit(IdrOut &O, uint32_t *win, const uint8_t *rbsp, long long len, int nal_byte, int as_nal, uint8_t *dst, long long cap, long long *len_out)
{
    return idr_unit_walk(O, win, rbsp, len, nal_byte, as_nal, dst, cap, 0, len_out);
}
/* the units of a picture's S slices behind each other in cap bytes: uoff[0 .. S) from ulen[0 .. S) (idr_unit_walk's counts; a negative
 * one: the slice could not be counted).  Returns 0 and the total, or PCAMV_ENOMEM / PCAMV_EINVAL with *total = 0: the slices of a picture
 * succeed or fail together */
SP_HD int idr_place(const long long *ulen, long long *uoff, int S, long long cap, long long *total)
{
    long long at = 0;
    *total = 0;
    for (int s = 0; s < S; s++) { if (ulen[s] < 0) return PCAMV_EINVAL; uoff[s] = at; at += ulen[s]; }
    if (at > cap) return PCAMV_ENOMEM;
    *total = at;
    return 0;
}
/* the prefix rule of a picture of several slices, serially (the definition k_idr_prefix_slices is held to by the host check): pre gets
 * n_mb + S entries, slice s's run at idr_slice_pre_at, its header's bits in front */
SP_HD int idr_prefix_slices(const IdrPic &P, const IdrSliceHdr *shdr, long long *pre)
{
    const int S = idr_n_slices(P.mb_h, P.slice_rows);
    int bad = 0;
    for (int s = 0; s < S; s++) {
        const int f = idr_slice_first_mb(P.mb_w, P.mb_h, P.slice_rows, s), n = idr_slice_n_mb(P.mb_w, P.mb_h, P.slice_rows, s);
        long long *q = pre + idr_slice_pre_at(f, s), at = shdr[s].bits;
        for (int k = 0; k < n; k++) { q[k] = at; if (P.bits[f + k] < 0) bad = 1; else at += P.bits[f + k]; }
        q[n] = at;
    }
    return bad;
}
#endif
