/*
 * pcamv_slice_write_cavlc.hip -- k_write_pslice_cavlc: a CAVLC P slice of every context's last step written on the device, one
 * wavefront per slice (gfx950).  The writer itself is pcamv_slice_write_cavlc.h (shared with the host test drivers); this unit gives
 * it its working memory -- LDS of the wave: a whole MBLocal, since a macroblock's levels are made here from its final motion with the
 * analysis' primitives, the CAVLC parser's neighbourhood and row buffer, the table block, the 26 per-lane block strings with their
 * lengths, an output buffer of SW_OBUF bytes -- and the slice's place in the batch.  Pictures wider than SP_LDS_COLS macroblocks keep
 * the row buffer in the wave's slot of a global scratch buffer.
 *
 * One wave per slice and thousands of slices in flight, as for k_write_pslice; inside a macroblock the 26 residual blocks are coded
 * by 26 lanes at once.  No spin-wait, no dependency between waves.  Bytes, length and status leave through ordinary vector stores;
 * the slice's place in the byte buffer is checked against the buffer here, every store against the slice's capacity by the writer.
 * A unit of its own for the reason pcamv_slice_write.hip gives: it inlines the analysis' primitives, and the other units compile as
 * before.  Nothing else is defined here.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pcamv_flow.hip.h"
#include "pcamv_slice_write_cavlc.h"

/* slice blockIdx.x: the last step of the context Fs[blockIdx.x] describes */
static __global__ void __launch_bounds__(64) k_write_pslice_cavlc(const FrameDev *__restrict__ Fs, const WriteJobs J)
{
    __shared__ MBLocal L;
    __shared__ uint32_t s_mv[48], s_tl[1], s_tab[SV_TAB_BYTES / 4], s_row[SP_LDS_COLS * SV_ROW_BYTES / 4], s_obuf[SW_OBUF / 4];
    __shared__ uint32_t s_blk[SWV_NBLK * SWV_BLK_DWORDS], s_blen[SWV_NBLK];
    __shared__ uint8_t s_nz[48];
    __shared__ int8_t s_ref[48];
    static_assert(SV_TAB_BYTES % 4 == 0 && SV_T_CBP % 4 == 0, "the table block is copied in dwords");
    const int i = blockIdx.x, lane = threadIdx.x;
    const FrameDev F = Fs[i];
    for (int k = lane; k < SV_TAB_BYTES / 4; k += 64) s_tab[k] = ((const uint32_t *)J.tab)[k];
    SP_SYNC();
    const int lds_cols = J.lds_cols < SP_LDS_COLS ? J.lds_cols : SP_LDS_COLS;
    SwvState W;
    SvState &S = W.S;
    S.win = nullptr; S.ctx = nullptr; S.cmvd = nullptr; S.cmv = s_mv; S.cref = s_ref; S.cnz = s_nz; S.tl = s_tl;
    S.vlc = (const uint16_t *)s_tab; S.cbp_of = (const uint8_t *)s_tab + SV_T_CBP;
    S.row = F.mb_w <= lds_cols ? (uint8_t *)s_row : J.scratch + (long long)i * J.scratch_stride;
    W.obuf = s_obuf; W.blk = s_blk; W.blen = s_blen;
    const int *hd = J.hdr + SW_HDR_WORDS * (J.n_hdr > 1 ? i : 0);
    const SwHeader H = {(const uint8_t *)J.hdr + hd[0], hd[1], hd[2], hd[3]};
    const long long off = J.off[i], cap = J.cap[i];
    long long len = 0;
    int rc = PCAMV_EINVAL;
    if (off >= 0 && cap >= 0 && cap <= J.bytes_size && off <= J.bytes_size - cap && (F.mb_w <= lds_cols || J.scratch))
        rc = pcamv_slice_write_cavlc(W, F, &L, J.mbs ? J.mbs : F.rec_mb, J.final && !J.mbs ? F.flip : nullptr, F.car_base, 16 * F.n_mb, H, J.as_nal,
                                     J.bytes + off, cap, &len);
    if (lane == 0) { J.status[i] = rc; J.len[i] = rc ? 0 : len; }
}

void pcamv_launch_write_pslice_cavlc(unsigned slices, hipStream_t st, const FrameDev *dF, const WriteJobs &J)
{
    hipLaunchKernelGGL(k_write_pslice_cavlc, dim3(slices), dim3(64), 0, st, dF, J);
}
