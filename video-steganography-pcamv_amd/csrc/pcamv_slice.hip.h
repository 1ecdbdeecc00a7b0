/*
 * pcamv_slice.hip.h -- k_parse_pslice, k_parse_pslice_cavlc: P slices parsed on the device, one wavefront per slice (gfx950).
 *
 * A CABAC slice is serial, like a CABAC frame in the analysis kernel; the answer is the same: one wave per slice, thousands of
 * slices in flight.  The parser itself is pcamv_slice_parse.h (shared with the host test drivers); this file gives it its working
 * memory -- LDS of the wave: byte window, context states, the two tables of the serial chain, the macroblock cache, the row
 * buffer -- and the slice's place in the batch.  The row buffer is in LDS for pictures up to SP_LDS_COLS macroblocks wide (2048
 * pixels: 6 KB, 7.8 KB per wave in all, 20 waves per CU), else in the wave's slot of a global scratch buffer (PCAMV_SLICE_LDS_COLS in the
 * environment of batch creation lowers the limit: how the tests reach that path with the pictures they have).
 *
 * No spin-wait, no dependency between waves: a slice that fails writes its status word and the wave is done.  Nothing depends on
 * a slice being well-formed: the slice's place in the byte buffer is checked against the buffer here, everything inside it by the
 * parser.  Records and status leave through ordinary vector stores.
 *
 * k_parse_pslice_cavlc is the same for --no-cabac streams (pcamv_slice_parse_cavlc.h).  A CAVLC slice has no context states and
 * no arithmetic decoder: the wave keeps the byte window, the VLC tables (one 16-bit entry per code), the macroblock cache and a row
 * buffer of 24 bytes per column -- 5044 bytes, so that LDS admits the 32 waves per CU the registers do.
 *
 * k_nal_to_rbsp is what runs in front of either parser when the receiver is handed NAL units: one wavefront per unit, lane-parallel
 * (pcamv_nal_unescape.h), the RBSP of unit i at the unit's own offset of a buffer of the library's.  The parsers do not know of it.
 *
 * k_write_pslice (pcamv_slice_write.hip) is the other direction: a CABAC P slice of every context's last step written on the device, one
 * wavefront per slice (pcamv_slice_write.h, which also describes a launch: WriteJobs).
 */
#ifndef PCAMV_SLICE_HIP_H
#define PCAMV_SLICE_HIP_H
#include "pcamv_embed.hip.h"
#include "pcamv_slice_parse.h"
#include "pcamv_slice_parse_cavlc.h"
#include "pcamv_nal_unescape.h"
#include "pcamv_slice_write.h"

/* the slices of one launch: slice i is bytes[off[i] .. off[i] + len[i]), its slice data starts behind bit start_bit[i], slice QP qp[i] */
struct SliceJobs {
    const uint8_t *bytes; long long bytes_size;
    const long long *off, *len, *start_bit; const int *qp;     /* (CAVLC reads no QP: qp is NULL there) */
    const uint8_t *tab;                 /* pcamv_entropy_tables.h in the block form of the parser: SP_TAB_BYTES of pcamv_slice_parse.h, or
                                         * SV_TAB_BYTES of pcamv_slice_parse_cavlc.h */
    uint8_t *scratch; long long scratch_stride;     /* row buffers of pictures wider than SP_LDS_COLS macroblocks, one per slice */
    int mb_w, mb_h;
    int lds_cols;                       /* <= SP_LDS_COLS: pictures wider than this many macroblocks use `scratch` */
};

/* slice blockIdx.x into Xs[blockIdx.x].mbs (n_mb = mb_w * mb_h records), its return code into *Xs[blockIdx.x].slice_status */
static __global__ void __launch_bounds__(64) k_parse_pslice(const ExtractDev *__restrict__ Xs, const SliceJobs J)
{
    __shared__ uint32_t s_win[64], s_mv[48], s_mvd[48], s_tl[1], s_tab[(256 + 512) / 4], s_row[SP_LDS_COLS * SP_ROW_BYTES / 4];
    __shared__ uint8_t s_ctx[SP_CTX_BYTES], s_nz[48];
    __shared__ int8_t s_ref[48];
    const int i = blockIdx.x, lane = threadIdx.x;
    const ExtractDev X = Xs[i];
    for (int k = lane; k < (256 + 512) / 4; k += 64) s_tab[k] = ((const uint32_t *)(J.tab + SP_TAB_TRANS))[k];
    SP_SYNC();
    const int lds_cols = J.lds_cols < SP_LDS_COLS ? J.lds_cols : SP_LDS_COLS;
    SpState S;
    S.win = s_win; S.ctx = s_ctx; S.cmv = s_mv; S.cmvd = s_mvd; S.cref = s_ref; S.cnz = s_nz; S.tl = s_tl;
    S.row = J.mb_w <= lds_cols ? (uint8_t *)s_row : J.scratch + (long long)i * J.scratch_stride;
    const SpTables T = {(const int8_t *)(J.tab + SP_TAB_INIT), (const uint8_t *)s_tab, (const uint8_t *)s_tab + 256};
    const long long off = J.off[i], len = J.len[i];
    int rc = PCAMV_EINVAL;
    if (off >= 0 && len >= 0 && len <= J.bytes_size && off <= J.bytes_size - len && X.n_mb == J.mb_w * J.mb_h && (J.mb_w <= lds_cols || J.scratch))
        rc = pcamv_slice_parse(S, T, J.bytes + off, len, J.start_bit[i], J.qp[i], J.mb_w, J.mb_h, (pcamv_mb_t *)X.mbs);
    if (lane == 0) *X.slice_status = rc;
}

/* the same for a CAVLC slice: J.tab is the SV_TAB_BYTES block, J.qp is not read, the scratch rows are SV_ROW_BYTES per column */
static __global__ void __launch_bounds__(64) k_parse_pslice_cavlc(const ExtractDev *__restrict__ Xs, const SliceJobs J)
{
    __shared__ uint32_t s_win[64], s_mv[48], s_tl[1], s_tab[SV_TAB_BYTES / 4], s_row[SP_LDS_COLS * SV_ROW_BYTES / 4];
    __shared__ uint8_t s_nz[48];
    __shared__ int8_t s_ref[48];
    static_assert(SV_TAB_BYTES % 4 == 0 && SV_T_CBP % 4 == 0, "the table block is copied and addressed in dwords");
    const int i = blockIdx.x, lane = threadIdx.x;
    const ExtractDev X = Xs[i];
    for (int k = lane; k < SV_TAB_BYTES / 4; k += 64) s_tab[k] = ((const uint32_t *)J.tab)[k];
    SP_SYNC();
    const int lds_cols = J.lds_cols < SP_LDS_COLS ? J.lds_cols : SP_LDS_COLS;
    SvState S;
    S.win = s_win; S.cmv = s_mv; S.cref = s_ref; S.cnz = s_nz; S.tl = s_tl;
    S.ctx = nullptr; S.cmvd = nullptr; S.trans = nullptr; S.rlps = nullptr;
    S.vlc = (const uint16_t *)s_tab; S.cbp_of = (const uint8_t *)s_tab + SV_T_CBP;
    S.row = J.mb_w <= lds_cols ? (uint8_t *)s_row : J.scratch + (long long)i * J.scratch_stride;
    const long long off = J.off[i], len = J.len[i];
    int rc = PCAMV_EINVAL;
    if (off >= 0 && len >= 0 && len <= J.bytes_size && off <= J.bytes_size - len && X.n_mb == J.mb_w * J.mb_h && (J.mb_w <= lds_cols || J.scratch))
        rc = pcamv_slice_parse_cavlc(S, J.bytes + off, len, J.start_bit[i], J.mb_w, J.mb_h, (pcamv_mb_t *)X.mbs);
    if (lane == 0) *X.slice_status = rc;
}

/* the NAL units of one launch: unit i is bytes[off[i] .. off[i] + len[i]); its RBSP goes to rbsp[off[i] ..) (a buffer of bytes_size bytes
 * too: an RBSP is shorter than its unit, so units that do not overlap give RBSPs that do not), the RBSP's length to rbsp_len[i] (-1: the
 * unit is invalid), its header byte to nal_header[i] (-1: it has none), its return code to status[i] */
struct NalJobs {
    const uint8_t *bytes; long long bytes_size;
    const long long *off, *len;
    uint8_t *rbsp; long long *rbsp_len; int *nal_header, *status;
};
static __global__ void __launch_bounds__(64) k_nal_to_rbsp(const NalJobs J)
{
    __shared__ uint32_t s_win[NU_WIN_DWORDS], s_out[NU_OUT_DWORDS];
    const int i = blockIdx.x, lane = threadIdx.x;
    const NuWork W = {s_win, s_out};
    const long long off = J.off[i], len = J.len[i];
    int rc = PCAMV_EINVAL;
    if (off >= 0 && len >= 0 && len <= J.bytes_size && off <= J.bytes_size - len)
        rc = pcamv_nal_unescape(W, J.bytes + off, len, J.rbsp + off, J.rbsp_len + i, J.nal_header + i);
    else if (lane == 0) { J.rbsp_len[i] = -1; J.nal_header[i] = -1; }
    if (lane == 0) J.status[i] = rc;
}
/* the writer's kernel is a unit of its own (pcamv_slice_write.hip): it inlines the analysis' prediction and transform primitives, and what
 * the compiler makes of the kernels of this unit depends on what else in the unit calls them */
void pcamv_launch_write_pslice(unsigned slices, hipStream_t st, const FrameDev *dF, const WriteJobs &J);
void pcamv_launch_write_pslice_cavlc(unsigned slices, hipStream_t st, const FrameDev *dF, const WriteJobs &J);   /* pcamv_slice_write_cavlc.hip */
#endif
