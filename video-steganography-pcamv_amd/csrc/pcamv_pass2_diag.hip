/*
 * pcamv_pass2_diag.hip -- the second pass and the loop filter with one launch per anti-diagonal, a block per macroblock (gfx950):
 * PCAMV_SCHED=diag launches both stages at once; pcamv_gpu_pass2_pframe hands out the unfiltered reconstruction in between, so it
 * launches them one after the other.  A macroblock goes through the same LDS tile as a task of k_pass2_deblock_flow, as a run of one
 * (pcamv_pass2.hip.h, NMAX = 1).  Nothing else is defined here.
 */
#include "pcamv_flow.hip.h"

/* the LDS of a block: the tile, and the head of the per-macroblock storage (PCAMV_PASS2_LDS: all the second pass touches of an MBLocal) */
struct P2DiagLDS { __attribute__((aligned(16))) uint8_t Lraw[PCAMV_PASS2_LDS]; __attribute__((aligned(16))) P2Unit U; };

/* STAGES = P2D_PASS2 | P2D_DEBLOCK: the filter of (x,y) only needs the pass-2 reconstruction of (x,y) itself and the filtered
 * neighbours of earlier diagonals, and only modifies macroblocks of earlier diagonals */
template <int STAGES>
static __global__ void __launch_bounds__(64) k_pass2_diag(const FrameDev *__restrict__ Fs, int d)
{
    __shared__ P2DiagLDS S;
    MBLocal *L = reinterpret_cast<MBLocal *>(S.Lraw);
    P2Unit *U = &S.U;
    const FrameDev F = Fs[blockIdx.y];
    int x, y;
    if (!diag_pos(F, d, &x, &y)) return;
    if (STAGES & P2D_PASS2) {
        p2_unit_load<1>(F, U, x, y, 1);
        if (mbk_pass2(F, L, x, y, p2_pre(U, 0))) p2_put_mb(U, L, 0);
    } else {
        /* the filter alone, after a kernel boundary: what it reads of the macroblock's MBLocal comes out of the frame as the first stage
         * left it -- the sixteen final MVs, one per lane (asked for with the tile), the type (the record's: the second pass never changes
         * it), the non-zero flags (with the tile); the reference is picture 0 */
        const int lane = LANE(), bx = lane & 3, by = (lane >> 2) & 3, c8 = SCAN8_0 + bx + 8 * by;
        uint32_t w = 0;
        if (lane < 16) w = NB_LD32(F.mv + 2 * ((4 * y + by) * 4 * F.mb_w + 4 * x + bx));
        p2_unit_load<1>(F, U, x, y, 1);
        L->i_type = U->rec[0].i_type; L->nnz_mask = U->nnz1[0];
        if (lane < 16) { L->cmv[c8][0] = (int16_t)(w & 0xffff); L->cmv[c8][1] = (int16_t)(w >> 16); L->cref[c8] = 0; }
        PCAMV_WAVE_SYNC();
    }
    if (STAGES & P2D_DEBLOCK) mbk_deblock_unit(F, U, L, 0, x, y);
    p2_unit_store<1>(F, U, x, y, 1);
}

void pcamv_launch_pass2_diag(int stages, unsigned blocks, unsigned gops, hipStream_t st, const FrameDev *dF, int d)
{
    if (stages == P2D_PASS2) hipLaunchKernelGGL(k_pass2_diag<P2D_PASS2>, dim3(blocks, gops), dim3(64), 0, st, dF, d);
    else if (stages == P2D_DEBLOCK) hipLaunchKernelGGL(k_pass2_diag<P2D_DEBLOCK>, dim3(blocks, gops), dim3(64), 0, st, dF, d);
    else hipLaunchKernelGGL(k_pass2_diag<P2D_PASS2 | P2D_DEBLOCK>, dim3(blocks, gops), dim3(64), 0, st, dF, d);
}
