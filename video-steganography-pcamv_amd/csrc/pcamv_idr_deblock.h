/*
 * pcamv_idr_deblock.h -- the loop filter of an IDR picture the device coded (pcamv_idr.h): control code that compiles for the device and
 * for the host.  On the device it is the body of k_idr_deblock (pcamv_idr.hip); on the host it is what tests/fuzz/check_idr_deblock.cpp
 * compiles with the scalar form of SP_LANES, to be compared with the library's sequential definition pcamv_gpu_deblock_intra_picture
 * (pcamv_mvsyntax.h), which stays the independent check: the two share no code and no table.  No HIP type.  Behind pcamv_slice_parse.h
 * (SP_HD, SP_LANES, SP_SYNC).
 *
 * Scope, fixed (8.7 for such a picture): a frame picture of one slice, intra macroblocks only -- Intra16x16, and with i4x4 Intra4x4
 * (pcamv_idr_i4x4.h) --, one QP, 4x4 transform, FilterOffsetA = FilterOffsetB = 0.  So nothing per macroblock is needed: with the 4x4
 * transform bS is 4 on the macroblock edges and 3 inside for every intra macroblock, whatever its type: 4 on a macroblock edge whose
 * neighbour lies in the picture, 3 on the three inner edges, and an edge on the picture's border is not filtered; indexA = indexB = QP for luma and the
 * chroma QP for both chroma planes.  alpha or beta 0 (index below 16) leaves every line alone: |a - b| < 0 never holds.
 *
 * One macroblock by one wavefront.  Staged in the wave's working memory: the macroblock with the four columns to its left and the four
 * rows above it -- luma 20 x 20, chroma 12 x 12 twice -- where they exist (mx > 0, my > 0); the corner above-left is neither read nor
 * written by any edge of this macroblock and is not staged.  The eight edges run in the standard's order, the four vertical ones left to
 * right, then the four horizontal ones top to bottom, a wave barrier between them; one line per lane, luma lines in lanes 0 .. 15, the
 * chroma lines of luma edges 0 and 2 in lanes 16 .. 31 (plane, line).  Stored back: the macroblock, the columns to its left (as dwords:
 * the fourth column goes back as it came) and the three rows above it.  Nothing outside the picture is read or written.
 *
 * Order between macroblocks: (x, y) needs (x - 1, y), (x, y - 1) and (x + 1, y - 1) filtered -- the last because that macroblock's left
 * edge changes three columns of (x, y - 1), whose lowest rows edge 0 of this one reads -- and is read by none of them afterwards: one
 * launch per anti-diagonal x + 2 y = d.  The macroblocks of one diagonal touch disjoint samples.
 */
#ifndef PCAMV_IDR_DEBLOCK_H
#define PCAMV_IDR_DEBLOCK_H
#include <stdint.h>

#define IDB_LP 20               /* the luma tile's pitch in bytes: 4 + 16 */
#define IDB_CP 12               /* a chroma tile's: 4 + 8 */
struct IdbWork { uint32_t y[IDB_LP * IDB_LP / 4], c[2][IDB_CP * IDB_CP / 4]; };
struct IdbPic { uint8_t *rec[3]; int mb_w, mb_h, qp, qpc; };      /* planes tightly packed; qpc: the chroma QP of both chroma planes */

/* Tables 8-16 / 8-17 at filter offsets 0: alpha(indexA), beta(indexB), tc0(indexA) of bS 3 */
SP_HD int idb_alpha(int i)
{
    constexpr uint8_t t[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90,
                               101, 113, 127, 144, 162, 182, 203, 226, 255, 255};
    return t[i];
}
SP_HD int idb_beta(int i)
{
    constexpr uint8_t t[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14,
                               15, 15, 16, 16, 17, 17, 18, 18};
    return t[i];
}
SP_HD int idb_tc0_bs3(int i)
{
    constexpr uint8_t t[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13,
                               14, 16, 18, 20, 23, 25};
    return t[i];
}
SP_HD int idb_abs(int v) { return v < 0 ? -v : v; }
SP_HD int idb_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* one line across an edge: q points at q0, the samples lie xs bytes apart.  bs 4 or 3; chroma lines change p0 and q0 only */
SP_HD void idb_line(uint8_t *q, int xs, int bs, int chroma, int alpha, int beta, int tc0)
{
    const int p1 = q[-2 * xs], p0 = q[-xs], q0 = q[0], q1 = q[xs];
    if (!(idb_abs(p0 - q0) < alpha && idb_abs(p1 - p0) < beta && idb_abs(q1 - q0) < beta)) return;
    if (chroma) {
        if (bs == 4) { q[-xs] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2); q[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2); return; }
        const int tc = tc0 + 1, delta = idb_clip(((q0 - p0) * 4 + (p1 - q1) + 4) >> 3, -tc, tc);
        q[-xs] = (uint8_t)idb_clip(p0 + delta, 0, 255); q[0] = (uint8_t)idb_clip(q0 - delta, 0, 255);
        return;
    }
    const int p2 = q[-3 * xs], q2 = q[2 * xs];
    const int ap = idb_abs(p2 - p0) < beta, aq = idb_abs(q2 - q0) < beta;
    if (bs == 4) {
        const int small = idb_abs(p0 - q0) < (alpha >> 2) + 2;
        if (small && ap) {
            const int p3 = q[-4 * xs];
            q[-xs] = (uint8_t)((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
            q[-2 * xs] = (uint8_t)((p2 + p1 + p0 + q0 + 2) >> 2);
            q[-3 * xs] = (uint8_t)((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
        } else q[-xs] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
        if (small && aq) {
            const int q3 = q[3 * xs];
            q[0] = (uint8_t)((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
            q[xs] = (uint8_t)((p0 + q0 + q1 + q2 + 2) >> 2);
            q[2 * xs] = (uint8_t)((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
        } else q[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
        return;
    }
    const int tc = tc0 + ap + aq, delta = idb_clip(((q0 - p0) * 4 + (p1 - q1) + 4) >> 3, -tc, tc);
    if (ap) q[-2 * xs] = (uint8_t)(p1 + idb_clip(((p2 + ((p0 + q0 + 1) >> 1)) >> 1) - p1, -tc0, tc0));
    if (aq) q[xs] = (uint8_t)(q1 + idb_clip(((q2 + ((p0 + q0 + 1) >> 1)) >> 1) - q1, -tc0, tc0));
    q[-xs] = (uint8_t)idb_clip(p0 + delta, 0, 255); q[0] = (uint8_t)idb_clip(q0 - delta, 0, 255);
}

/* dword k of the staged area, k < 172: luma 20 rows of 5 dwords, then per chroma plane 12 rows of 3.  The tile's dword, the plane's
 * offset; false where the picture has no such samples, for the corner above-left, or (store) for what no edge of this macroblock
 * changes: the fourth row above */
SP_HD bool idb_slot(const IdbPic &P, int k, int mx, int my, bool store, int *pl, int *at, size_t *off)
{
    const int c = k < 100 ? 0 : k < 136 ? 1 : 2, kk = k - (c == 0 ? 0 : c == 1 ? 100 : 136);
    const int n = c ? 8 : 16, dw = c ? 3 : 5, r = kk / dw - 4, x = 4 * (kk % dw) - 4;
    if ((r < 0 && (my == 0 || x < 0)) || (x < 0 && mx == 0) || (store && r == -4)) return false;
    const size_t w = (size_t)n * P.mb_w;
    *pl = c; *at = kk;
    *off = (size_t)((long long)n * my + r) * w + (size_t)((long long)n * mx + x);
    return true;
}

/* macroblock (mx, my) of P, by one wavefront: the macroblocks of the anti-diagonals x + 2 y before this one's are done */
SP_HD void idr_deblock_mb(IdbWork &W, const IdbPic &P, int mx, int my)
{
    const int alpha = idb_alpha(P.qp), beta = idb_beta(P.qp), tc0 = idb_tc0_bs3(P.qp);
    const int calpha = idb_alpha(P.qpc), cbeta = idb_beta(P.qpc), ctc0 = idb_tc0_bs3(P.qpc);
    if (!((alpha && beta) || (calpha && cbeta))) return;           /* no line of this picture can change */
    uint8_t *ty = (uint8_t *)W.y;
    SP_SYNC();
    SP_LANES(l)
        for (int k = l; k < 172; k += 64) {
            int pl, at; size_t off;
            if (idb_slot(P, k, mx, my, false, &pl, &at, &off)) (pl ? W.c[pl - 1] : W.y)[at] = *(const uint32_t *)(P.rec[pl] + off);
        }
    SP_SYNC();
    for (int dir = 0; dir < 2; dir++)
        for (int edge = 0; edge < 4; edge++) {
            const int bs = edge ? 3 : (dir ? my : mx) > 0 ? 4 : 0;
            if (bs)
                SP_LANES(l) {
                    if (l < 16) {
                        if (alpha && beta) {
                            uint8_t *q = dir == 0 ? ty + (l + 4) * IDB_LP + 4 * edge + 4 : ty + (4 * edge + 4) * IDB_LP + l + 4;
                            idb_line(q, dir == 0 ? 1 : IDB_LP, bs, 0, alpha, beta, tc0);
                        }
                    } else if (l < 32 && !(edge & 1) && calpha && cbeta) {
                        uint8_t *tc = (uint8_t *)W.c[(l - 16) >> 3];
                        const int cl = (l - 16) & 7;
                        uint8_t *q = dir == 0 ? tc + (cl + 4) * IDB_CP + 2 * edge + 4 : tc + (2 * edge + 4) * IDB_CP + cl + 4;
                        idb_line(q, dir == 0 ? 1 : IDB_CP, bs, 1, calpha, cbeta, ctc0);
                    }
                }
            SP_SYNC();
        }
    SP_LANES(l)
        for (int k = l; k < 172; k += 64) {
            int pl, at; size_t off;
            if (idb_slot(P, k, mx, my, true, &pl, &at, &off)) *(uint32_t *)(P.rec[pl] + off) = (pl ? W.c[pl - 1] : W.y)[at];
        }
    SP_SYNC();
}

/* the macroblocks of anti-diagonal d = x + 2 y: rows y_lo .. y_hi (empty: y_hi < y_lo), x = d - 2 y */
SP_HD void idb_diag_rows(int d, int mb_w, int mb_h, int *y_lo, int *y_hi)
{
    *y_lo = d - (mb_w - 1) > 0 ? (d - (mb_w - 1) + 1) >> 1 : 0;
    *y_hi = (d >> 1) < mb_h - 1 ? d >> 1 : mb_h - 1;
}
SP_HD int idb_n_diag(int mb_w, int mb_h) { return mb_w + 2 * (mb_h - 1); }
#endif
