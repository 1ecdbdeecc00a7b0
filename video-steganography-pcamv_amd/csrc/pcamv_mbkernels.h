/*
 * pcamv_mbkernels.h -- per-macroblock bodies of the three analysis phases.
 *
 *   phase A  mbk_search : motion search + partition decision of one MB.  MB(x,y) needs the final
 *                         motion of its left, top-left, top and top-right neighbours
 *                         (common/macroblock.c:28-163, 422-439), so MBs on the anti-diagonal
 *                         x + 2y = d are independent and diagonals run in order.
 *   phase B  mbk_rca    : replacement-MV cost of ONE carrier MV (x264_ih_get_mv_cost,
 *                         analyse.c:2391-2550): 1 + up to 12 whole-MB re-encodes, 9 SATDs each.
 *                         Depends only on that MB's own decision -> embarrassingly parallel.
 *   phase C  mbk_encode : the pass-1 reconstruction of the MB (encoder/macroblock.c:484).
 */
#ifndef PCAMV_MBKERNELS_H
#define PCAMV_MBKERNELS_H
#include "pcamv_logic.h"

#ifdef PCAMV_HOST_EMU
#define PCAMV_LANE0 1
#else
#define PCAMV_LANE0 (LANE() == 0)
#endif

/* what follows the decision: (--subme >= 6) the pass-1 reconstruction and the entropy coder's bookkeeping, then the record and the
 * macroblock's final motion, written through for the neighbours */
template <int VARIANT>
PCAMV_DEV void mbk_search_finish(const FrameDev &F, MBLocal *L, Analysis *a, int mb_x, int mb_y)
{
    if (MBRD_ON) {
        /* --subme >= 6: the macroblock as coded is part of what its neighbours read (reconstructed pixels for the intra
         * thresholds, non-zero flags / coded block pattern / MV differences / context states for the bit counts), so the
         * pass-1 reconstruction and the entropy coder's bookkeeping come before the hand-off */
        const unsigned long long t_c = PROF_T();
        L->b_skip_mc = 0;
        /* the trial of the decided mode has produced all of it already, unless no trial ran (P_SKIP, modes beyond the
         * thresholds) or the kept one is another mode */
        const int kept = L->i_type != PCAMV_P_SKIP && L->snap_part == L->i_partition;
        if (kept) prim_rd_restore(F, L);
        else mb_encode(F, L, 0, 1);
#ifdef PCAMV_HOST_EMU
        prim_store_rec(F, L);
#else
        prim_store_rec(F, L, true);
#endif
        if (PCAMV_LANE0 && FD(F).nnz) FD(F).nnz[L->mb_xy] = (uint16_t)L->nnz_mask;      /* with the pixels: what pass 2 takes over for a macroblock the embedding leaves alone */
        entropy_commit(F, L, kept);
        PROF_ADD(22, t_c);
    }
    const unsigned long long t_w = PROF_T();
    const int xy = L->mb_xy;
    int *slots = L->slots;
    const int used = F.embed && L->i_type != PCAMV_P_SKIP;
    const int n = carrier_slots(L->i_type, L->i_partition, L->sub_part, used, slots);
    pcamv_mb_t *r = &FD(F).rec_mb[xy];
    const int s4 = 4 * F.mb_w, s8 = 2 * F.mb_w, b4 = 4 * (mb_y * s4 + mb_x), b8 = 2 * (mb_y * s8 + mb_x);
    PCAMV_WAVE_SYNC();
    /* the 16 per-4x4 entries of the record and of the frame's motion field (x264_macroblock_cache_save,
     * common/macroblock.c:1254-1364), one per lane */
    FOR_CAND(i, 16) {
        int i8 = scan8_of(i);
        r->ref[i] = L->cref[i8]; r->mv[i][0] = L->cmv[i8][0]; r->mv[i][1] = L->cmv[i8][1];
        r->mv_stego[i][0] = r->mv_stego[i][1] = 0; r->inter_stego_cost[i] = 0;
        int x = i & 3, y = i >> 2;
        NB_ST32(&FD(F).mv[2 * (b4 + y * s4 + x)], NB_PACK16(L->cmv[SCAN8_0 + x + 8 * y][0], L->cmv[SCAN8_0 + x + 8 * y][1]));
    }
    if (PCAMV_LANE0) {
        r->i_type = L->i_type; r->i_partition = L->i_partition; r->i_qp = FD(F).qp;
        for (int i = 0; i < 4; i++) r->i_sub_partition[i] = L->i_type == PCAMV_P_8x8 ? L->sub_part[i] : PCAMV_D_L0_8x8;
        r->pskip_mv[0] = L->pskip_mv[0]; r->pskip_mv[1] = L->pskip_mv[1];
        if (L->i_type != PCAMV_P_SKIP) { r->mvr16[0] = L->mvr_own[0]; r->mvr16[1] = L->mvr_own[1]; }
        else { r->mvr16[0] = r->mvr16[1] = 0; }
        r->used = (uint8_t)used; r->pad[0] = r->pad[1] = r->pad[2] = 0;
        for (int k = 0; k < n; k++) {
            MEState *me = slot_me(L, a, slots[k]);
            FD(F).mvp_aux[(xy * 16 + slots[k]) * 2] = (int16_t)me->mvp[0];
            FD(F).mvp_aux[(xy * 16 + slots[k]) * 2 + 1] = (int16_t)me->mvp[1];
        }
        NB_ST8(&FD(F).mb_type[xy], L->i_type);
        NB_ST16(&FD(F).ref8[b8], (uint16_t)(uint8_t)L->cref[scan8_of(0)] | (uint16_t)(uint8_t)L->cref[scan8_of(4)] << 8);
        NB_ST16(&FD(F).ref8[b8 + s8], (uint16_t)(uint8_t)L->cref[scan8_of(8)] | (uint16_t)(uint8_t)L->cref[scan8_of(12)] << 8);
    }
    PROF_ADD(12, t_w);
}
template <int VARIANT>
PCAMV_DEV void mbk_search(const FrameDev &F, MBLocal *L, Analysis *a, int mb_x, int mb_y)
{
    const unsigned long long t_l = PROF_T();
    if ((VARIANT & (V_TESA | V_RD)) == (V_TESA | V_RD) && F.b_mbrd) {
        /* --me tesa with the RD mode decision: the Hadamard exhaustive search keeps its survivor list in the LDS the RD stage keeps
         * the context states in (TESA_SLOT / L_CAB), so what the RD stage needs from memory is fetched after the searches, not with
         * the macroblock's other loads */
        mb_load(F, L, mb_x, mb_y, false, 0);
        PROF_ADD(11, t_l);
        const int skip = analyse_s16<VARIANT>(F, L, a);
        if (!skip) analyse_s_rest<VARIANT>(F, L, a);
        { MbFetch pf; prim_mb_fetch(F, mb_x, mb_y, L->neighbour, 1, pf); prim_mb_fetch_store(F, L, 1, pf); }
        if (!skip) analyse_decide<VARIANT>(F, L, a);
        update_cache(L, a);
    } else {
        mb_load(F, L, mb_x, mb_y, false, MBRD_ON);
        PROF_ADD(11, t_l);
        analyse_mb_search<VARIANT>(F, L, a);
    }
    mbk_search_finish<VARIANT>(F, L, a, mb_x, mb_y);
}

/* rebuild the decided partitioning (types, MVs, search-time mvp) from the record */
PCAMV_DEV int analysis_from_record(const FrameDev &F, MBLocal *L, Analysis *a, int xy, int *slots)
{
    const pcamv_mb_t *r = &FD(F).rec_mb[xy];
    mb_load(F, L, xy % F.mb_w, xy / F.mb_w);
    L->i_type = r->i_type; L->i_partition = r->i_partition;
    for (int i = 0; i < 4; i++) L->sub_part[i] = r->i_sub_partition[i];
    const int n = carrier_slots(L->i_type, L->i_partition, L->sub_part, L->i_type != PCAMV_P_SKIP, slots);
    for (int k = 0; k < n; k++) {
        int s = slots[k], ip, xo, yo;
        MEState *me = slot_me(L, a, s);
        slot_geometry(L->i_type, L->i_partition, L->sub_part, s, &ip, &xo, &yo);
        me_setup(me, ip, xo, yo);
        me->mv[0] = r->mv[s][0]; me->mv[1] = r->mv[s][1];
        me->mvp[0] = FD(F).mvp_aux[(xy * 16 + s) * 2]; me->mvp[1] = FD(F).mvp_aux[(xy * 16 + s) * 2 + 1];
    }
    return n;
}

PCAMV_DEV void mbk_rca(const FrameDev &F, MBLocal *L, Analysis *a, int xy, int k)
{
    if (!FD(F).rec_mb[xy].used) return;
    int *slots = L->slots;
    const int n = analysis_from_record(F, L, a, xy, slots);
    if (k >= n) return;
    MEState *me = slot_me(L, a, slots[k]);
    int dx = 0, dy = 0;
    const int bx = me->mv[0], by = me->mv[1];
    const int cost = rca_mv_cost(F, L, a, me, &dx, &dy, 0);
    if (PCAMV_LANE0) {
        pcamv_mb_t *r = &FD(F).rec_mb[xy];
        r->mv_stego[slots[k]][0] = (int16_t)(bx + dx); r->mv_stego[slots[k]][1] = (int16_t)(by + dy);
        r->inter_stego_cost[slots[k]] = cost;
    }
}

/* phases C + B of one macroblock back to back (dataflow schedule): the pass-1 reconstruction, then
 * every carrier's replacement-MV cost.  The reconstruction of the macroblock as decided is also the
 * first re-encode of every carrier's RCA step, so it is made once (L->recb0); rca_mv_cost leaves the
 * decided MVs and the cache as it found them, so one rebuild of the analysis serves all carriers. */
/* fused = this wave has just searched this macroblock (dataflow schedule): MBLocal and Analysis still hold what
 * analysis_from_record would rebuild from the record (neighbour cache, limits, source pixels, decided MVs in the cache,
 * the carriers' search states), so only the fields that call resets are reset */
PCAMV_DEV int mbk_recon(const FrameDev &F, MBLocal *L, Analysis *a, int xy, int fused = 0, int have_rec = 0)
{
    const unsigned long long t_e = PROF_T();
    int n;
    if (fused) {
        L->b_skip_mc = 0;
        n = carrier_slots(L->i_type, L->i_partition, L->sub_part, L->i_type != PCAMV_P_SKIP, L->slots);
        for (int k = 0; k < n; k++) { MEState *me = slot_me(L, a, L->slots[k]); me->cost = me->cost_mv = me->cost_rec = 0; }
        if (have_rec) { PROF_ADD(10, t_e); return n; }      /* the search phase has reconstructed and stored the macroblock already (L->pred) */
    } else {
        n = analysis_from_record(F, L, a, xy, L->slots);
        update_cache(L, a);
    }
    mb_encode(F, L);
    prim_store_rec(F, L);
    if (PCAMV_LANE0 && FD(F).nnz) FD(F).nnz[xy] = (uint16_t)L->nnz_mask;
    PROF_ADD(10, t_e);
    return n;
}
PCAMV_DEV void mbk_rca_all(const FrameDev &F, MBLocal *L, Analysis *a, int xy, int n)
{
    int *slots = L->slots;
    if (FD(F).rec_mb[xy].used && n > 0) {
        const unsigned long long t_w = PROF_T();
        PROF_CNT(42, n);
        prim_copy_pred(L, L->recb0);
        /* a 16x16 macroblock whose RCA neighbourhood (+-3 quarter pels) needs no MV clipping reads its
         * reference pixels from an LDS window loaded once, instead of ~30 scattered global fetches */
        int win = 0;
        if (L->i_type == PCAMV_P_L0 && L->i_partition == PCAMV_D_16x16) {
            const int bx = a->me16x16.mv[0], by = a->me16x16.mv[1];
            if (bx - 3 >= L->mv_min[0] && bx + 3 <= L->mv_max[0] && by - 3 >= L->mv_min[1] && by + 3 <= L->mv_max[1]) { prim_win_load(F, L, bx, by); win = 1; }
        }
        PROF_ADD(34, t_w);
        for (int k = 0; k < n; k++) {
            MEState *me = slot_me(L, a, slots[k]);
            int dx = 0, dy = 0;
            const int bx = me->mv[0], by = me->mv[1];
            const int cost = rca_mv_cost(F, L, a, me, &dx, &dy, 1, win);
            if (PCAMV_LANE0) {
                pcamv_mb_t *r = &FD(F).rec_mb[xy];
                r->mv_stego[slots[k]][0] = (int16_t)(bx + dx); r->mv_stego[slots[k]][1] = (int16_t)(by + dy);
                r->inter_stego_cost[slots[k]] = cost;
            }
        }
    }
}
PCAMV_DEV void mbk_rca_encode(const FrameDev &F, MBLocal *L, Analysis *a, int xy, int fused = 0, int have_rec = 0)
{
    mbk_rca_all(F, L, a, xy, mbk_recon(F, L, a, xy, fused, have_rec));
}

PCAMV_DEV void mbk_encode(const FrameDev &F, MBLocal *L, Analysis *a, int xy)
{
    analysis_from_record(F, L, a, xy, L->slots);
    update_cache(L, a);
    mb_encode(F, L);
    prim_store_rec(F, L);
    if (PCAMV_LANE0 && FD(F).nnz) FD(F).nnz[xy] = (uint16_t)L->nnz_mask;
}
#endif
