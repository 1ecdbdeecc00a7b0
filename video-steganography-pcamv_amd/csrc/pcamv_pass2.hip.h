/*
 * pcamv_pass2.hip.h -- the loop filter and the second pass' tile of a run of macroblocks (gfx950): types and __device__ functions
 * only.  Every unit of the library sees this header through pcamv_flow.hip.h (flow_loop's second-pass arm names P2Unit), so it
 * holds no kernel; the kernels that use it are the main unit's (pcamv_kernels.hip.h).
 *
 *   mbk_deblock         the loop filter of one macroblock in a staging area of its own (the per-diagonal kernels)
 *   p2_unit_load / p2_put_mb / mbk_deblock_unit / p2_unit_store   the same for a run of up to eight macroblocks of a row held as
 *                       one tile in LDS (P2Unit; k_pass2_deblock_flow)
 */
#ifndef PCAMV_PASS2_HIP_H
#define PCAMV_PASS2_HIP_H
#include "pcamv_common.h"
#include "pcamv_prims_gpu.h"
#include "pcamv_mbkernels.h"

/* H.264 Tables 8-16 / 8-17: alpha(indexA), beta(indexB), tc0(indexA, bS = 1..3) */
__device__ static const uint8_t dbk_alpha_dev[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28,
                                                     32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255};
__device__ static const uint8_t dbk_beta_dev[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8,
                                                    9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18};
__device__ static const int8_t dbk_tc0_dev[52][3] = {
    {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0},
    {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 1, 1}, {0, 1, 1}, {1, 1, 1},
    {1, 1, 1}, {1, 1, 1}, {1, 1, 1}, {1, 1, 2}, {1, 1, 2}, {1, 1, 2}, {1, 1, 2}, {1, 2, 3}, {1, 2, 3}, {2, 2, 3}, {2, 2, 4}, {2, 3, 4},
    {2, 3, 4}, {3, 3, 5}, {3, 4, 6}, {3, 4, 6}, {4, 5, 7}, {4, 5, 8}, {4, 6, 9}, {5, 7, 10}, {6, 8, 11}, {6, 8, 13}, {7, 10, 14}, {8, 11, 16},
    {9, 12, 18}, {10, 13, 20}, {11, 15, 23}, {13, 17, 25}};

/* Loop filter of one macroblock (x264_frame_deblock_row, common/frame.c:627-798, inter macroblocks, 4x4
 * transform, one QP): the macroblock and the 4 pixels left of / above it are staged in LDS, the 32
 * boundary strengths are computed one per lane, then the four vertical and the four horizontal edges are
 * filtered in order (one line per lane: 16 luma, 8 + 8 chroma on even edges) and the touched pixels go back.
 * Needs (x-1,y), (x,y-1) and (x+1,y-1) filtered: same anti-diagonal order as the search. */
struct DeblockLDS { uint8_t sy[20][24]; uint8_t sc[2][12][16]; uint8_t sbs[2][4][4]; };
/* Lo: the MBLocal pass 2 of this macroblock has just run in (same wave): its unfiltered reconstruction (pred), type, final
 * motion and non-zero flags are taken from there; nullptr: everything is in memory like the neighbours' */
__device__ __forceinline__ void mbk_deblock(const FrameDev &F, DeblockLDS *D, int mx, int my, const MBLocal *Lo = nullptr)
{
    const uint8_t *own = Lo ? Lo->pred : nullptr;
    uint8_t (*sy)[24] = D->sy;              /* rows / cols -4..15 of the macroblock at [r + 4][c + 4] */
    uint8_t (*sc)[12][16] = D->sc;          /* chroma rows / cols -4..7 */
    uint8_t (*sbs)[4][4] = D->sbs;
    const int lane = LANE(), xy = my * F.mb_w + mx, W = F.w, CW = F.w >> 1;
    const int gx = 16 * mx, gy = 16 * my, cgx = 8 * mx, cgy = 8 * my;
    /* stage: 20 rows x 5 dwords of luma, 2 x 12 rows x 3 dwords of chroma (nothing outside the picture) */
    for (int i = lane; i < 100; i += 64) {
        const int r = i / 5 - 4, c = (i % 5) * 4 - 4;
        if (own && r >= 0 && c >= 0) *(uint32_t *)&sy[r + 4][c + 4] = lds4(own + r * 16 + c);
        else if (gy + r >= 0 && gx + c >= 0) *(uint32_t *)&sy[r + 4][c + 4] = NB_LD32(F.rec[0] + (size_t)(gy + r) * W + gx + c);
    }
    for (int i = lane; i < 72; i += 64) {
        const int pl = i / 36, j = i % 36, r = j / 3 - 4, c = (j % 3) * 4 - 4;
        if (own && r >= 0 && c >= 0) *(uint32_t *)&sc[pl][r + 4][c + 4] = lds4(own + 256 + r * 16 + pl * 8 + c);
        else if (cgy + r >= 0 && cgx + c >= 0) *(uint32_t *)&sc[pl][r + 4][c + 4] = NB_LD32((pl ? F.rec[2] : F.rec[1]) + (size_t)(cgy + r) * CW + cgx + c);
    }
    /* boundary strengths */
    const int type = Lo ? Lo->i_type : (int)NB_LD8(&F.mb_type[xy]), qp = F.qp;
    const int qp_thresh = 15 - (F.chroma_qp_offset > 0 ? F.chroma_qp_offset : 0);
    const int edge_end = (type == PCAMV_P_SKIP || qp <= qp_thresh) ? 1 : 4;
    const int no_sub8x8 = type != PCAMV_P_8x8 || !(F.inter & PCAMV_ANALYSE_PSUB8x8);
    if (lane < 32) {
        const int dir = lane >> 4, edge = (lane >> 2) & 3, i = lane & 3;
        int bs = 0;
        const bool on = edge < edge_end && !(edge == 0 && (dir ? my == 0 : mx == 0));
        if (on) {
            const int x = dir == 0 ? edge : i, y = dir == 0 ? i : edge;
            const int xn = dir == 0 ? (x - 1) & 3 : x, yn = dir == 0 ? y : (y - 1) & 3;
            const int nxy = edge ? xy : (dir ? xy - F.mb_w : xy - 1);
            const int bi = (x & 1) + 2 * (y & 1) + 4 * (x >> 1) + 8 * (y >> 1), bn = (xn & 1) + 2 * (yn & 1) + 4 * (xn >> 1) + 8 * (yn >> 1);
            const int s4 = 4 * F.mb_w, s8 = 2 * F.mb_w;
            const int fx = 4 * mx + x, fy = 4 * my + y, fxn = dir == 0 ? fx - 1 : fx, fyn = dir == 0 ? fy : fy - 1;
            /* both sides of the edge: flags, motion, reference -- this macroblock's from LDS when it has just been made
             * here, the rest in one round of loads (not one per test) */
            const bool nb_local = Lo && edge;
            const int c8a = SCAN8_0 + x + 8 * y, c8b = SCAN8_0 + xn + 8 * yn;
            const unsigned nz_a = Lo ? (unsigned)Lo->nnz_mask : (unsigned)NB_LD16(&F.nnz[xy]);
            const unsigned nz_b = nb_local ? (unsigned)Lo->nnz_mask : (unsigned)NB_LD16(&F.nnz[nxy]);
            const uint32_t wa = Lo ? NB_PACK16(Lo->cmv[c8a][0], Lo->cmv[c8a][1]) : NB_LD32(F.mv + 2 * (fy * s4 + fx));
            const uint32_t wb = nb_local ? NB_PACK16(Lo->cmv[c8b][0], Lo->cmv[c8b][1]) : NB_LD32(F.mv + 2 * (fyn * s4 + fxn));
            const int ra = Lo ? (int)Lo->cref[c8a] : (int)NB_LD8(&F.ref8[(fy >> 1) * s8 + (fx >> 1)]);
            const int rb = nb_local ? (int)Lo->cref[c8b] : (int)NB_LD8(&F.ref8[(fyn >> 1) * s8 + (fxn >> 1)]);
            if (((nz_a >> bi) & 1) || ((nz_b >> bn) & 1)) bs = 2;
            else if (!(edge & no_sub8x8)) {
                const int a0 = (int16_t)(wa & 0xffff), a1 = (int16_t)(wa >> 16), b0 = (int16_t)(wb & 0xffff), b1 = (int16_t)(wb >> 16);
                if (ra != rb || iabs(a0 - b0) >= 4 || iabs(a1 - b1) >= 4) bs = 1;
                bs |= 0x10;              /* marks "decided by the motion test" for the copy rule below */
            }
        }
        sbs[dir][edge][i] = (uint8_t)bs;
    }
    __syncthreads();
    {   /* frame.c:735-737: inside an 8x8 that cannot be split, the odd 4-pixel group repeats its left/upper
         * neighbour's strength unless that one is 2 */
        const int dir = (lane >> 4) & 1, edge = (lane >> 2) & 3, i = lane & 3;
        int bs = sbs[dir][edge][i];
        const int prev = i ? sbs[dir][edge][i - 1] & 0xf : 0;
        __syncthreads();
        if (lane < 32) {
            if ((bs & 0x10) && (i & no_sub8x8) && prev != 2) bs = prev;
            sbs[dir][edge][i] = (uint8_t)(bs & 0xf);
        }
    }
    __syncthreads();
    const int qpc = F.chroma_qp;
    const int alpha = dbk_alpha_dev[qp], beta = dbk_beta_dev[qp], calpha = dbk_alpha_dev[qpc], cbeta = dbk_beta_dev[qpc];
    /* tc0 of the three strengths, looked up once (a per-edge table load would sit on the chain of eight dependent edges) */
    const int tl1 = dbk_tc0_dev[qp][0], tl2 = dbk_tc0_dev[qp][1], tl3 = dbk_tc0_dev[qp][2];
    const int tc1 = dbk_tc0_dev[qpc][0], tc2 = dbk_tc0_dev[qpc][1], tc3 = dbk_tc0_dev[qpc][2];
    for (int dir = 0; dir < 2; dir++)
        for (int edge = 0; edge < 4; edge++) {
            const uint32_t any = *(const uint32_t *)sbs[dir][edge];
            if (any) {
                if (lane < 16 && alpha && beta) {
                    const int bs = sbs[dir][edge][lane >> 2];
                    if (bs) {
                        const int tc0 = bs == 1 ? tl1 : bs == 2 ? tl2 : tl3;
                        uint8_t *q = dir == 0 ? &sy[lane + 4][4 * edge + 4] : &sy[4 * edge + 4][lane + 4];
                        const int xs = dir == 0 ? 1 : 24;
                        const int p2 = q[-3 * xs], p1 = q[-2 * xs], p0 = q[-xs], q0 = q[0], q1 = q[xs], q2 = q[2 * xs];
                        if (iabs(p0 - q0) < alpha && iabs(p1 - p0) < beta && iabs(q1 - q0) < beta) {
                            int tc = tc0;
                            if (iabs(p2 - p0) < beta) { q[-2 * xs] = (uint8_t)(p1 + clip3i(((p2 + ((p0 + q0 + 1) >> 1)) >> 1) - p1, -tc0, tc0)); tc++; }
                            if (iabs(q2 - q0) < beta) { q[xs] = (uint8_t)(q1 + clip3i(((q2 + ((p0 + q0 + 1) >> 1)) >> 1) - q1, -tc0, tc0)); tc++; }
                            const int delta = clip3i((((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc);
                            q[-xs] = (uint8_t)clip3i(p0 + delta, 0, 255); q[0] = (uint8_t)clip3i(q0 - delta, 0, 255);
                        }
                    }
                } else if (lane >= 16 && lane < 32 && !(edge & 1) && calpha && cbeta) {
                    const int pl = (lane - 16) >> 3, l = (lane - 16) & 7, bs = sbs[dir][edge][l >> 1];
                    if (bs) {
                        const int tc = (bs == 1 ? tc1 : bs == 2 ? tc2 : tc3) + 1;
                        uint8_t *q = dir == 0 ? &sc[pl][l + 4][2 * edge + 4] : &sc[pl][2 * edge + 4][l + 4];
                        const int xs = dir == 0 ? 1 : 16;
                        const int p1 = q[-2 * xs], p0 = q[-xs], q0 = q[0], q1 = q[xs];
                        if (iabs(p0 - q0) < calpha && iabs(p1 - p0) < cbeta && iabs(q1 - q0) < cbeta) {
                            const int delta = clip3i((((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc);
                            q[-xs] = (uint8_t)clip3i(p0 + delta, 0, 255); q[0] = (uint8_t)clip3i(q0 - delta, 0, 255);
                        }
                    }
                }
            }
            __syncthreads();
        }
    /* write back: the macroblock, the 4 columns left of it (rows 0..15), the 4 rows above it (cols 0..15) */
    { const int r = lane >> 2, c = (lane & 3) * 4;
      NB_ST32(F.rec[0] + (size_t)(gy + r) * W + gx + c, *(const uint32_t *)&sy[r + 4][c + 4]); }
    if (lane < 16 && mx > 0) NB_ST32(F.rec[0] + (size_t)(gy + lane) * W + gx - 4, *(const uint32_t *)&sy[lane + 4][0]);
    if (lane >= 16 && lane < 32 && my > 0) { const int r = (lane - 16) >> 2, c = ((lane - 16) & 3) * 4;
      NB_ST32(F.rec[0] + (size_t)(gy - 4 + r) * W + gx + c, *(const uint32_t *)&sy[r][c + 4]); }
    if (lane >= 32) {
        const int pl = (lane - 32) >> 4, j = (lane - 32) & 15, r = j >> 1, c = (j & 1) * 4;
        uint8_t *dst = pl ? F.rec[2] : F.rec[1];
        NB_ST32(dst + (size_t)(cgy + r) * CW + cgx + c, *(const uint32_t *)&sc[pl][r + 4][c + 4]);
    }
    __syncthreads();
    if (lane < 16 && mx > 0) { const int pl = lane >> 3, r = lane & 7; uint8_t *dst = pl ? F.rec[2] : F.rec[1];
      NB_ST32(dst + (size_t)(cgy + r) * CW + cgx - 4, *(const uint32_t *)&sc[pl][r + 4][0]); }
    if (lane >= 16 && lane < 32 && my > 0) { const int pl = (lane - 16) >> 3, j = (lane - 16) & 7, r = j >> 1, c = (j & 1) * 4; uint8_t *dst = pl ? F.rec[2] : F.rec[1];
      NB_ST32(dst + (size_t)(cgy - 4 + r) * CW + cgx + c, *(const uint32_t *)&sc[pl][r][c + 4]); }
}
/* ------------------------------------------------------------------ the second pass of a RUN of macroblocks of a row (k_pass2_deblock_flow)
 * A task of the second-pass kernel is up to eight macroblocks of a row.  Taken one by one, each cost two or three memory round trips (record,
 * pixels, the filter's borders), fetched 4 KB for its 0.6 KB (a macroblock's sixteen 16-byte rows are sixteen cache lines, which its seven
 * neighbours in the run fetch again) and stored its rows as partial lines.  Here the run is ONE tile in LDS: its pixels with the four
 * rows above and the four columns to the left (rows of up to 132 bytes: whole lines), the eight records and the neighbours' side of the
 * outer edges come in one round trip; the macroblocks are then reconstructed (where the embedding changed them) and filtered in place, the
 * left neighbour's side of an edge handed from one to the next in LDS; the tile goes back in rows. */
#define P2_TW 144        /* tile row pitch, luma: columns -4 .. 127 at [c + 4] */
#define P2_CW 80         /* chroma: columns -4 .. 63 at [c + 4] */
struct P2Unit {
    uint8_t ty[20][P2_TW];              /* rows -4 .. 15 at [r + 4] */
    uint8_t tc[2][12][P2_CW];
    pcamv_mb_t rec[8];
    int car_base[8], mbflip[8], nnz1[8];
    unsigned t_nnz[8]; uint32_t t_mv[8][4]; int t_ref[8][4];      /* the upper neighbours' bottom row of 4x4 blocks */
    unsigned l_nnz; uint32_t l_mv[4]; int l_ref[4];                 /* the left neighbour's right column: of the run's first macroblock from memory, then handed on */
    uint8_t sbs[2][4][4];
};
#define P2_LSLOTS (20 * 33)             /* luma dwords of the tile: row r = i / 33 - 4, column c = 4 * (i % 33) - 4 */
#define P2_CSLOTS (2 * 12 * 17)         /* chroma: plane i / 204, row (i % 204) / 17 - 4, column 4 * (i % 17) - 4 */
__device__ __forceinline__ bool p2_slot(const FrameDev &F, int i, bool chroma, int x0, int y, int n, int *pl, int *r, int *c, size_t *goff)
{
    if (!chroma) {
        if (i >= P2_LSLOTS) return false;
        *pl = 0; *r = i / 33 - 4; *c = 4 * (i % 33) - 4;
        const int gx = 16 * x0 + *c, gy = 16 * y + *r;
        if (gx < 0 || gy < 0 || *c >= 16 * n) return false;
        *goff = (size_t)gy * F.w + gx;
    } else {
        if (i >= P2_CSLOTS) return false;
        const int j = i % 204;
        *pl = 1 + i / 204; *r = j / 17 - 4; *c = 4 * (j % 17) - 4;
        const int gx = 8 * x0 + *c, gy = 8 * y + *r;
        if (gx < 0 || gy < 0 || *c >= 8 * n) return false;
        *goff = (size_t)gy * (F.w >> 1) + gx;
    }
    return true;
}
__device__ __forceinline__ void p2_unit_load(const FrameDev &F, P2Unit *U, int x0, int y, int n)
{
    const int lane = LANE(), xy0 = y * F.mb_w + x0;
    /* every load first, then the stores to LDS: one round trip for the run */
    uint32_t vl[11], vc[7], vr[8];
#pragma unroll
    for (int t = 0; t < 11; t++) {
        int pl, r, c; size_t o;
        vl[t] = p2_slot(F, lane + 64 * t, false, x0, y, n, &pl, &r, &c, &o) ? NB_LD32(F.rec[0] + o) : 0u;
    }
#pragma unroll
    for (int t = 0; t < 7; t++) {
        int pl, r, c; size_t o;
        vc[t] = 0u;
        if (p2_slot(F, lane + 64 * t, true, x0, y, n, &pl, &r, &c, &o)) vc[t] = NB_LD32((pl == 2 ? F.rec[2] : F.rec[1]) + o);
    }
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const int i = lane + 64 * t, k = i / 59, w = i - 59 * k;
        vr[t] = (i < 8 * 59 && k < n) ? ((const uint32_t *)&F.rec_mb[xy0 + k])[w] : 0u;
    }
    int cb = 0, mf = 1, n1 = 0;
    if (lane < n) { cb = F.car_base ? F.car_base[xy0 + lane] : 0; mf = F.mbflip ? (int)F.mbflip[xy0 + lane] : 1; n1 = (int)F.nnz[xy0 + lane]; }
    unsigned tn = 0, ln = 0; uint32_t tm = 0, lm = 0; int tr = 0, lr = 0;
    const int s4 = 4 * F.mb_w, s8 = 2 * F.mb_w;
    if (lane < 4 * n && y > 0) {          /* lane = 4 k + j: block j of the bottom row of the macroblock above macroblock k */
        const int k = lane >> 2, j = lane & 3, fx = 4 * (x0 + k) + j, fy = 4 * y - 1;
        tn = (unsigned)NB_LD16(&F.nnz[xy0 + k - F.mb_w]); tm = NB_LD32(F.mv + 2 * (fy * s4 + fx)); tr = (int)NB_LD8(&F.ref8[(fy >> 1) * s8 + (fx >> 1)]);
    }
    if (lane >= 32 && lane < 36 && x0 > 0) {      /* block (3, j) of the macroblock left of the run */
        const int j = lane - 32, fx = 4 * x0 - 1, fy = 4 * y + j;
        ln = (unsigned)NB_LD16(&F.nnz[xy0 - 1]); lm = NB_LD32(F.mv + 2 * (fy * s4 + fx)); lr = (int)NB_LD8(&F.ref8[(fy >> 1) * s8 + (fx >> 1)]);
    }
    PCAMV_WAVE_SYNC();
#pragma unroll
    for (int t = 0; t < 11; t++) {
        int pl, r, c; size_t o;
        if (p2_slot(F, lane + 64 * t, false, x0, y, n, &pl, &r, &c, &o)) *(uint32_t *)&U->ty[r + 4][c + 4] = vl[t];
    }
#pragma unroll
    for (int t = 0; t < 7; t++) {
        int pl, r, c; size_t o;
        if (p2_slot(F, lane + 64 * t, true, x0, y, n, &pl, &r, &c, &o)) *(uint32_t *)&U->tc[pl - 1][r + 4][c + 4] = vc[t];
    }
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const int i = lane + 64 * t;
        if (i < 8 * 59) ((uint32_t *)U->rec)[i] = vr[t];
    }
    if (lane < 8) { U->car_base[lane] = cb; U->mbflip[lane] = mf; U->nnz1[lane] = n1; }
    if (lane < 32) { U->t_mv[lane >> 2][lane & 3] = tm; U->t_ref[lane >> 2][lane & 3] = tr; if ((lane & 3) == 0) U->t_nnz[lane >> 2] = tn; }
    if (lane >= 32 && lane < 36) { U->l_mv[lane - 32] = lm; U->l_ref[lane - 32] = lr; if (lane == 32) U->l_nnz = ln; }
    PCAMV_WAVE_SYNC();
}
/* a reconstructed macroblock (L->pred) into its place in the tile */
__device__ __forceinline__ void p2_put_mb(P2Unit *U, const MBLocal *L, int k)
{
    const int lane = LANE();
    PCAMV_WAVE_SYNC();
    *(uint32_t *)&U->ty[(lane >> 2) + 4][16 * k + 4 + 4 * (lane & 3)] = lds4(L->pred + (lane >> 2) * 16 + (lane & 3) * 4);
    if (lane < 32) *(uint32_t *)&U->tc[lane >> 4][((lane & 15) >> 1) + 4][8 * k + 4 + 4 * (lane & 1)] = lds4(L->pred + 256 + ((lane & 15) >> 1) * 16 + (lane >> 4) * 8 + (lane & 1) * 4);
    PCAMV_WAVE_SYNC();
}
/* the loop filter of macroblock k of the run, in the tile (what mbk_deblock does in its staging area; same strengths, same arithmetic) */
__device__ __forceinline__ void mbk_deblock_unit(const FrameDev &F, P2Unit *U, const MBLocal *Lo, int k, int mx, int my)
{
    uint8_t (*sbs)[4][4] = U->sbs;
    const int lane = LANE();
    const int type = Lo->i_type, qp = F.qp;
    const int qp_thresh = 15 - (F.chroma_qp_offset > 0 ? F.chroma_qp_offset : 0);
    const int edge_end = (type == PCAMV_P_SKIP || qp <= qp_thresh) ? 1 : 4;
    const int no_sub8x8 = type != PCAMV_P_8x8 || !(F.inter & PCAMV_ANALYSE_PSUB8x8);
    PCAMV_WAVE_SYNC();
    if (lane < 32) {
        const int dir = lane >> 4, edge = (lane >> 2) & 3, i = lane & 3;
        int bs = 0;
        const bool on = edge < edge_end && !(edge == 0 && (dir ? my == 0 : mx == 0));
        if (on) {
            const int x = dir == 0 ? edge : i, y = dir == 0 ? i : edge;
            const int xn = dir == 0 ? (x - 1) & 3 : x, yn = dir == 0 ? y : (y - 1) & 3;
            const int bi = (x & 1) + 2 * (y & 1) + 4 * (x >> 1) + 8 * (y >> 1), bn = (xn & 1) + 2 * (yn & 1) + 4 * (xn >> 1) + 8 * (yn >> 1);
            const int c8a = SCAN8_0 + x + 8 * y, c8b = SCAN8_0 + xn + 8 * yn;
            const unsigned nz_a = (unsigned)Lo->nnz_mask;
            const unsigned nz_b = edge ? (unsigned)Lo->nnz_mask : dir ? U->t_nnz[k] : U->l_nnz;
            const uint32_t wa = NB_PACK16(Lo->cmv[c8a][0], Lo->cmv[c8a][1]);
            const uint32_t wb = edge ? NB_PACK16(Lo->cmv[c8b][0], Lo->cmv[c8b][1]) : dir ? U->t_mv[k][i] : U->l_mv[i];
            const int ra = (int)Lo->cref[c8a];
            const int rb = edge ? (int)Lo->cref[c8b] : dir ? U->t_ref[k][i] : U->l_ref[i];
            if (((nz_a >> bi) & 1) || ((nz_b >> bn) & 1)) bs = 2;
            else if (!(edge & no_sub8x8)) {
                const int a0 = (int16_t)(wa & 0xffff), a1 = (int16_t)(wa >> 16), b0 = (int16_t)(wb & 0xffff), b1 = (int16_t)(wb >> 16);
                if (ra != rb || iabs(a0 - b0) >= 4 || iabs(a1 - b1) >= 4) bs = 1;
                bs |= 0x10;
            }
        }
        sbs[dir][edge][i] = (uint8_t)bs;
    }
    __syncthreads();
    {
        const int dir = (lane >> 4) & 1, edge = (lane >> 2) & 3, i = lane & 3;
        int bs = sbs[dir][edge][i];
        const int prev = i ? sbs[dir][edge][i - 1] & 0xf : 0;
        __syncthreads();
        if (lane < 32) {
            if ((bs & 0x10) && (i & no_sub8x8) && prev != 2) bs = prev;
            sbs[dir][edge][i] = (uint8_t)(bs & 0xf);
        }
    }
    __syncthreads();
    const int qpc = F.chroma_qp;
    const int alpha = dbk_alpha_dev[qp], beta = dbk_beta_dev[qp], calpha = dbk_alpha_dev[qpc], cbeta = dbk_beta_dev[qpc];
    const int tl1 = dbk_tc0_dev[qp][0], tl2 = dbk_tc0_dev[qp][1], tl3 = dbk_tc0_dev[qp][2];
    const int tc1 = dbk_tc0_dev[qpc][0], tc2 = dbk_tc0_dev[qpc][1], tc3 = dbk_tc0_dev[qpc][2];
    /* luma lines in lanes 0..15, the chroma lines of the even edges in lanes 16..31 (plane, line), ONE instruction stream for both: the chroma
     * filter is the luma one without the second-neighbour terms and with tc = tc0 + 1 (deblock_chroma_c vs deblock_luma_c, common/frame.c) */
    const bool is_c = lane >= 16;
    const int cpl = (lane - 16) >> 3, cl = (lane - 16) & 7;
    const int f_alpha = is_c ? calpha : alpha, f_beta = is_c ? cbeta : beta;
    for (int dir = 0; dir < 2; dir++)
        for (int edge = 0; edge < 4; edge++) {
            const uint32_t any = *(const uint32_t *)sbs[dir][edge];
            if (any) {
                if (lane < 32 && f_alpha && f_beta && !(is_c && (edge & 1))) {
                    const int bs = sbs[dir][edge][is_c ? cl >> 1 : lane >> 2];
                    if (bs) {
                        const int tc0 = is_c ? (bs == 1 ? tc1 : bs == 2 ? tc2 : tc3) : (bs == 1 ? tl1 : bs == 2 ? tl2 : tl3);
                        uint8_t *q = is_c ? (dir == 0 ? &U->tc[cpl][cl + 4][8 * k + 2 * edge + 4] : &U->tc[cpl][2 * edge + 4][8 * k + cl + 4])
                                          : (dir == 0 ? &U->ty[lane + 4][16 * k + 4 * edge + 4] : &U->ty[4 * edge + 4][16 * k + lane + 4]);
                        const int xs = dir == 0 ? 1 : is_c ? P2_CW : P2_TW;
                        const int p2 = q[-3 * xs], p1 = q[-2 * xs], p0 = q[-xs], q0 = q[0], q1 = q[xs], q2 = q[2 * xs];
                        if (iabs(p0 - q0) < f_alpha && iabs(p1 - p0) < f_beta && iabs(q1 - q0) < f_beta) {
                            const bool ap = !is_c && iabs(p2 - p0) < f_beta, aq = !is_c && iabs(q2 - q0) < f_beta;
                            const int tc = is_c ? tc0 + 1 : tc0 + (ap ? 1 : 0) + (aq ? 1 : 0);
                            if (ap) q[-2 * xs] = (uint8_t)(p1 + clip3i(((p2 + ((p0 + q0 + 1) >> 1)) >> 1) - p1, -tc0, tc0));
                            if (aq) q[xs] = (uint8_t)(q1 + clip3i(((q2 + ((p0 + q0 + 1) >> 1)) >> 1) - q1, -tc0, tc0));
                            const int delta = clip3i((((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc);
                            q[-xs] = (uint8_t)clip3i(p0 + delta, 0, 255); q[0] = (uint8_t)clip3i(q0 - delta, 0, 255);
                        }
                    }
                }
            }
            __syncthreads();
        }
    /* this macroblock's right column of 4x4 blocks is the next one's left neighbour */
    if (lane < 4) { const int c8 = SCAN8_0 + 3 + 8 * lane; U->l_mv[lane] = NB_PACK16(Lo->cmv[c8][0], Lo->cmv[c8][1]); U->l_ref[lane] = (int)Lo->cref[c8]; }
    if (lane == 0) U->l_nnz = (unsigned)Lo->nnz_mask;
    PCAMV_WAVE_SYNC();
}
/* the tile back to the frame: the run's rows 0..15 with the four columns left of it (the left neighbour's, touched by the first
 * macroblock's left edge), and the four rows above it */
__device__ __forceinline__ void p2_unit_store(const FrameDev &F, P2Unit *U, int x0, int y, int n)
{
    const int lane = LANE();
    PCAMV_WAVE_SYNC();
#pragma unroll
    for (int t = 0; t < 11; t++) {
        int pl, r, c; size_t o;
        if (p2_slot(F, lane + 64 * t, false, x0, y, n, &pl, &r, &c, &o) && (r < 0 ? c >= 0 : true)) NB_ST32(F.rec[0] + o, *(const uint32_t *)&U->ty[r + 4][c + 4]);
    }
#pragma unroll
    for (int t = 0; t < 7; t++) {
        int pl, r, c; size_t o;
        if (p2_slot(F, lane + 64 * t, true, x0, y, n, &pl, &r, &c, &o) && (r < 0 ? c >= 0 : true)) NB_ST32((pl == 2 ? F.rec[2] : F.rec[1]) + o, *(const uint32_t *)&U->tc[pl - 1][r + 4][c + 4]);
    }
}
#endif
