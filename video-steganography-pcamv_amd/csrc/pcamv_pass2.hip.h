/*
 * pcamv_pass2.hip.h -- the second pass and the loop filter of a run of macroblocks of a row, held as one tile in LDS (gfx950): types
 * and __device__ functions only.  Every unit of the library sees this header through pcamv_flow.hip.h (flow_loop's second-pass arm
 * is made of these functions), so it holds no kernel; the kernels that use it are k_pass2_deblock_flow (main unit, pcamv_kernels.hip.h) with
 * runs of up to eight macroblocks and the per-diagonal kernels (pcamv_pass2_diag.hip) with runs of one.
 *
 *   p2_unit_load / p2_unit_store   the tile (P2Unit) in from the frame and back
 *   mbk_pass2 / p2_put_mb          the second pass of one macroblock of the run; its new reconstruction into the tile
 *   mbk_deblock_unit               the loop filter of one macroblock, in the tile -- the only loop filter of the library
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

/* ------------------------------------------------------------------ the second pass of a RUN of macroblocks of a row (k_pass2_deblock_flow; runs of one: pcamv_pass2_diag.hip)
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
/* NMAX: the longest run the caller hands in (8: a task of k_pass2_deblock_flow; 1: the per-diagonal kernels) -- the tile's dwords are walked
 * 64 at a time, and only as many of them as a run of NMAX has */
#define P2_LROW(NMAX) (4 * (NMAX) + 1)              /* luma dwords of a tile row: row r = i / P2_LROW - 4, column c = 4 * (i % P2_LROW) - 4 */
#define P2_CROW(NMAX) (2 * (NMAX) + 1)              /* chroma: plane i / (12 * P2_CROW), row (i % (12 * P2_CROW)) / P2_CROW - 4, column 4 * (i % P2_CROW) - 4 */
#define P2_LITER(NMAX) ((20 * P2_LROW(NMAX) + 63) / 64)
#define P2_CITER(NMAX) ((2 * 12 * P2_CROW(NMAX) + 63) / 64)
#define P2_RITER(NMAX) ((59 * (NMAX) + 63) / 64)    /* the records: 59 words each */
template <int NMAX>
__device__ __forceinline__ bool p2_slot(const FrameDev &F, int i, bool chroma, int x0, int y, int n, int *pl, int *r, int *c, size_t *goff)
{
    if (!chroma) {
        if (i >= 20 * P2_LROW(NMAX)) return false;
        *pl = 0; *r = i / P2_LROW(NMAX) - 4; *c = 4 * (i % P2_LROW(NMAX)) - 4;
        const int gx = 16 * x0 + *c, gy = 16 * y + *r;
        if (gx < 0 || gy < 0 || *c >= 16 * n) return false;
        *goff = (size_t)gy * F.w + gx;
    } else {
        if (i >= 2 * 12 * P2_CROW(NMAX)) return false;
        const int j = i % (12 * P2_CROW(NMAX));
        *pl = 1 + i / (12 * P2_CROW(NMAX)); *r = j / P2_CROW(NMAX) - 4; *c = 4 * (j % P2_CROW(NMAX)) - 4;
        const int gx = 8 * x0 + *c, gy = 8 * y + *r;
        if (gx < 0 || gy < 0 || *c >= 8 * n) return false;
        *goff = (size_t)gy * (F.w >> 1) + gx;
    }
    return true;
}
template <int NMAX = 8>
__device__ __forceinline__ void p2_unit_load(const FrameDev &F, P2Unit *U, int x0, int y, int n)
{
    const int lane = LANE(), xy0 = y * F.mb_w + x0;
    /* every load first, then the stores to LDS: one round trip for the run */
    uint32_t vl[P2_LITER(NMAX)], vc[P2_CITER(NMAX)], vr[P2_RITER(NMAX)];
#pragma unroll
    for (int t = 0; t < P2_LITER(NMAX); t++) {
        int pl, r, c; size_t o;
        vl[t] = p2_slot<NMAX>(F, lane + 64 * t, false, x0, y, n, &pl, &r, &c, &o) ? NB_LD32(F.rec[0] + o) : 0u;
    }
#pragma unroll
    for (int t = 0; t < P2_CITER(NMAX); t++) {
        int pl, r, c; size_t o;
        vc[t] = 0u;
        if (p2_slot<NMAX>(F, lane + 64 * t, true, x0, y, n, &pl, &r, &c, &o)) vc[t] = NB_LD32((pl == 2 ? F.rec[2] : F.rec[1]) + o);
    }
#pragma unroll
    for (int t = 0; t < P2_RITER(NMAX); t++) {
        const int i = lane + 64 * t, k = i / 59, w = i - 59 * k;
        vr[t] = (i < NMAX * 59 && k < n) ? ((const uint32_t *)&F.rec_mb[xy0 + k])[w] : 0u;
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
    for (int t = 0; t < P2_LITER(NMAX); t++) {
        int pl, r, c; size_t o;
        if (p2_slot<NMAX>(F, lane + 64 * t, false, x0, y, n, &pl, &r, &c, &o)) *(uint32_t *)&U->ty[r + 4][c + 4] = vl[t];
    }
#pragma unroll
    for (int t = 0; t < P2_CITER(NMAX); t++) {
        int pl, r, c; size_t o;
        if (p2_slot<NMAX>(F, lane + 64 * t, true, x0, y, n, &pl, &r, &c, &o)) *(uint32_t *)&U->tc[pl - 1][r + 4][c + 4] = vc[t];
    }
#pragma unroll
    for (int t = 0; t < P2_RITER(NMAX); t++) {
        const int i = lane + 64 * t;
        if (i < NMAX * 59) ((uint32_t *)U->rec)[i] = vr[t];
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
/* pass 2 of one macroblock of the run (analyse.c:2870-3107 + x264_macroblock_encode, semantics of DESIGN.md 5b): the
 * pass-1 type / partition, the record's MVs with mv_stego where the flip map says so, for a P_SKIP
 * macroblock the skip prediction from the FINAL neighbours; reconstruction; final motion + non-zero flags
 * for the loop filter and for the next frame's temporal candidates.  Same left / top / top-right
 * dependency as the search. */
/* What the macroblock needs of memory came in with the tile (P2Pre, out of P2Unit): the record, the index of the first carrier, "any
 * carrier flipped", the first pass' non-zero flags; and the pixels of a macroblock the embedding left alone are already where the loop
 * filter works -- nothing is loaded here then.  Returns 1 when the macroblock was reconstructed anew (L->pred holds its pixels, for
 * p2_put_mb), 0 when the first pass' reconstruction stands. */
struct P2Pre { const pcamv_mb_t *r; int base, any_flip, nnz1, drain; };
__device__ __forceinline__ P2Pre p2_pre(const P2Unit *U, int k)
{
    P2Pre pre;
    pre.r = &U->rec[k]; pre.base = U->car_base[k]; pre.any_flip = U->mbflip[k]; pre.nnz1 = U->nnz1[k]; pre.drain = k > 0;
    return pre;
}
__device__ __forceinline__ int mbk_pass2(const FrameDev &F, MBLocal *L, int mb_x, int mb_y, const P2Pre &unit)
{
    const int xy = mb_y * F.mb_w + mb_x;
    const pcamv_mb_t *r = unit.r;
    PCAMV_WAVE_SYNC();
    /* (a later macroblock of the run: the skip prediction reads the left neighbour's final motion from memory, where this wave stored it a moment ago) */
    if (unit.drain && r->i_type == PCAMV_P_SKIP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    /* only a skipped macroblock needs its neighbours (skip prediction); the source pixels only a macroblock that is re-encoded (below) */
    const bool coded = r->i_type != PCAMV_P_SKIP;
    mb_load(F, L, mb_x, mb_y, coded);
    L->i_type = r->i_type; L->i_partition = r->i_partition;
    for (int i = 0; i < 4; i++) L->sub_part[i] = r->i_sub_partition[i];
    cache_ref_set(L, 0, 0, 4, 4, 0);
    int same;
    if (L->i_type == PCAMV_P_SKIP) {
        L->i_partition = PCAMV_D_16x16;
        cache_mv_set(L, 0, 0, 4, 4, L->pskip_mv[0], L->pskip_mv[1]);
        same = L->pskip_mv[0] == r->pskip_mv[0] && L->pskip_mv[1] == r->pskip_mv[1];
    } else {
        int *slots = L->slots;
        const int n = carrier_slots(L->i_type, L->i_partition, L->sub_part, r->used, slots);
        const int base = unit.base;
        PCAMV_WAVE_SYNC();
        /* its carriers' flip flags: one more round trip, for the macroblocks that have a flipped carrier at all */
        if (rfl(unit.any_flip)) { FOR_CAND(j, n) L->cxy[j] = FD(F).flip ? (uint32_t)(FD(F).flip[base + j] == 1) : 0u; }
        else { FOR_CAND(j, n) L->cxy[j] = 0u; }
        PCAMV_WAVE_SYNC();
        FOR_CAND(i, 16) {
            const int s = carrier_of_block(L->i_type, L->i_partition, L->sub_part, i);
            int flipped = 0;
            for (int j = 0; j < n; j++) if (slots[j] == s) flipped = (int)L->cxy[j];
            L->cmv[scan8_of(i)][0] = flipped ? r->mv_stego[s][0] : r->mv[i][0];
            L->cmv[scan8_of(i)][1] = flipped ? r->mv_stego[s][1] : r->mv[i][1];
        }
        PCAMV_WAVE_SYNC();
        same = 1;
        for (int j = 0; j < n; j++) if (L->cxy[j]) same = 0;
    }
    /* A macroblock whose motion is what the first pass decided -- no carrier of it flipped; skipped with the same skip prediction --
     * reconstructs to what the first pass stored (same type, motion, source, reference and quantiser): pixels and non-zero flags
     * are taken from there instead of being made again.  (~7 of 8 macroblocks at half a bit per carrier.) */
    const int reuse = same && FD(F).rec_is_pass1;
    if (reuse) L->nnz_mask = unit.nnz1;
    else {
        if (coded) prim_load_fenc(F, L);
        mb_encode(F, L);
    }
    /* final motion, type and non-zero flags: read by the neighbours' skip prediction and loop filter in the same
     * launch, so stored write-through like the search's hand-off */
    const int s4 = 4 * F.mb_w, s8 = 2 * F.mb_w, b4 = 4 * (mb_y * s4 + mb_x), b8 = 2 * (mb_y * s8 + mb_x);
    PCAMV_WAVE_SYNC();
    FOR_CAND(i, 16) {
        int x = i & 3, y = i >> 2;
        NB_ST32(&FD(F).mv[2 * (b4 + y * s4 + x)], NB_PACK16(L->cmv[SCAN8_0 + x + 8 * y][0], L->cmv[SCAN8_0 + x + 8 * y][1]));
    }
    if (LANE() == 0) {
        NB_ST8(&FD(F).mb_type[xy], L->i_type);
        NB_ST16(&FD(F).ref8[b8], 0); NB_ST16(&FD(F).ref8[b8 + s8], 0);
        NB_ST16(&FD(F).nnz[xy], L->nnz_mask);
    }
    return !reuse;
}
/* The loop filter of macroblock k of the run, in the tile (x264_frame_deblock_row, common/frame.c:627-798, inter macroblocks, 4x4
 * transform, one QP): the 32 boundary strengths are computed one per lane, then the four vertical and the four horizontal edges are
 * filtered in order, one line per lane.  Needs (x-1,y), (x,y-1) and (x+1,y-1) filtered: same anti-diagonal order as the search.
 * Of Lo -- the MBLocal pass 2 of this macroblock has just run in -- it reads type, final motion (cmv, cref) and non-zero flags. */
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
template <int NMAX = 8>
__device__ __forceinline__ void p2_unit_store(const FrameDev &F, P2Unit *U, int x0, int y, int n)
{
    const int lane = LANE();
    PCAMV_WAVE_SYNC();
#pragma unroll
    for (int t = 0; t < P2_LITER(NMAX); t++) {
        int pl, r, c; size_t o;
        if (p2_slot<NMAX>(F, lane + 64 * t, false, x0, y, n, &pl, &r, &c, &o) && (r < 0 ? c >= 0 : true)) NB_ST32(F.rec[0] + o, *(const uint32_t *)&U->ty[r + 4][c + 4]);
    }
#pragma unroll
    for (int t = 0; t < P2_CITER(NMAX); t++) {
        int pl, r, c; size_t o;
        if (p2_slot<NMAX>(F, lane + 64 * t, true, x0, y, n, &pl, &r, &c, &o) && (r < 0 ? c >= 0 : true)) NB_ST32((pl == 2 ? F.rec[2] : F.rec[1]) + o, *(const uint32_t *)&U->tc[pl - 1][r + 4][c + 4]);
    }
}
#endif
