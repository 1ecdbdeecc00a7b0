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
 * k_stream_plan, k_stream_scan, k_stream_prefix, k_stream_place cut every context's Annex B byte stream into its NAL units, a wavefront
 * per chunk of a stream (pcamv_stream_index.h); k_stream_unit then takes one slice unit per context and call from the table and
 * unescapes it with k_nal_to_rbsp's control code, k_slice_header reads its slice header, one lane per context, into the job arrays the
 * parsers read, and k_stream_status puts the code of the first stage that failed where the parser put its own.  k_stream_window_unit
 * takes a window of units per context instead, one wavefront per unit, for the same kernels over contexts x slots jobs.
 *
 * k_pset_unit, k_pset_parse, k_pset_resolve read every stream's SPS / PPS units into one table of parameter sets per context
 * (pcamv_param_sets.h; the units are found by the instances of k_stream_scan / k_stream_prefix / k_stream_place made for SI_SEL_PSET), and
 * k_slice_header_sets is k_slice_header under those tables in place of one parameter set for the batch.
 *
 * k_write_pslice (pcamv_slice_write.hip) is the other direction: a CABAC P slice of every context's last step written on the device, one
 * wavefront per slice (pcamv_slice_write.h, which also describes a launch: WriteJobs).
 *
 * k_stream_open, k_stream_slot, k_stream_commit put that writer's units into one Annex B byte stream per context (pcamv_stream_write.h), one
 * lane per context: k_stream_slot in front of the writer makes each picture's slice header in the header table the writer reads and gives
 * the writer its place at the stream's end, k_stream_commit behind it moves the stream's end over what was written.
 *
 * k_stream_open_heads, k_stream_join, k_stream_copy_plan, k_stream_copy and k_video_cut make one video of many chains (pcamv_video.h): a
 * head of its own at the start of every context's stream, the contexts' streams behind each other in one video -- both through
 * k_stream_copy, a wavefront per chunk of a job's destination -- and on the receiving side a video's table of units walked by one
 * wavefront into the contexts' (off, len), which the index kernels take from there.  k_video_prefix_local / _top / _apply are
 * k_stream_prefix for that one long stream, in two levels on many wavefronts.  k_pset_spread gives every context the video's sets.
 */
#ifndef PCAMV_SLICE_HIP_H
#define PCAMV_SLICE_HIP_H
#include "pcamv_embed.hip.h"
#include "pcamv_slice_parse.h"
#include "pcamv_slice_parse_cavlc.h"
#include "pcamv_nal_unescape.h"
#include "pcamv_stream_index.h"
#include "pcamv_param_sets.h"
#include "pcamv_slice_write.h"
#include "pcamv_stream_write.h"
#include "pcamv_video.h"

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

/* ---- byte streams.  The index of n streams: stream i is bytes[off[i] .. off[i] + len[i]); its chunks' summaries are chunks[chunk_base[i]
 * .. chunk_base[i + 1]) (k_stream_plan: room for max_chunks in all; a stream that does not fit the buffer or the room has bad[i] set and
 * no chunk); its table is table[i * stride .. + max_units) */
struct StreamJobs {
    const uint8_t *bytes; long long bytes_size;
    const long long *off, *len;
    long long *chunk_base; int *bad; SiChunk *chunks; long long max_chunks;
    pcamv_unit_t *table; long long max_units, stride; int all;
    long long *n_units, *n_slices, *cursor; unsigned long long *longest;
    int n;
};
/* sel -- 0: the slice units; SI_SEL_PSET: the parameter-set units are what is counted and listed -- is a constant of each instance of the
 * three kernels below, so the instances the index call launches hold no trace of the other selection */
SP_HD SiTable stream_table(const StreamJobs &J, int i, int sel) { const SiTable T = {J.table + (long long)i * J.stride, J.max_units, J.all, J.longest, sel}; return T; }
/* one wavefront: the chunks of every stream, their exclusive prefix.  Lane l owns streams [l * seg, (l + 1) * seg) and walks them one
 * after the other, so the kernel's time grows linearly with n (0.04 ms at 4096 streams): beyond some 10^5 streams of one call a scan over
 * several waves would be the next step */
static __global__ void __launch_bounds__(64) k_stream_plan(const StreamJobs J)
{
    __shared__ long long s_sum[64];
    const int lane = threadIdx.x, seg = (J.n + 63) / 64, i0 = lane * seg, i1 = i0 + seg < J.n ? i0 + seg : J.n;
    long long sum = 0;
    for (int i = i0; i < i1; i++) {
        const long long off = J.off[i], len = J.len[i];
        if (off >= 0 && len >= 0 && len <= J.bytes_size && off <= J.bytes_size - len) sum += si_chunks(J.bytes + off, len);
    }
    s_sum[lane] = sum;
    __syncthreads();
    long long base = 0;
    for (int j = 0; j < lane; j++) base += s_sum[j];
    for (int i = i0; i < i1; i++) {
        const long long off = J.off[i], len = J.len[i];
        const int fits = off >= 0 && len >= 0 && len <= J.bytes_size && off <= J.bytes_size - len;
        const long long c = fits ? si_chunks(J.bytes + off, len) : 0;
        const int bad = !fits || base + c > J.max_chunks;
        J.chunk_base[i] = base; J.bad[i] = bad;
        if (!bad) base += c;
        if (bad) { J.n_units[i] = PCAMV_EINVAL; J.n_slices[i] = PCAMV_EINVAL; }
        J.cursor[i] = 0;
    }
    /* (chunk_base[i + 1] is read as stream i's end only where stream i is not bad: stream_chunks) */
}
/* the stream flat chunk f belongs to and its number there; -1: none (the grid is sized for the most chunks there can be).  Streams
 * without chunks (empty, or bad) share their base with the stream behind them, and the walk down over them is one step per such
 * stream: a long run of empty streams in front of a long one costs every wave of the long one that many steps */
static __device__ int stream_of_chunk(const StreamJobs &J, long long f, long long *c)
{
    int lo = 0, hi = J.n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (J.chunk_base[mid] <= f) lo = mid; else hi = mid - 1; }
    /* streams without chunks share their base with the next one: the last stream at or below f that has chunk f is the one */
    while (lo >= 0) {
        if (!J.bad[lo]) {
            const long long n = si_chunks(J.bytes + J.off[lo], J.len[lo]);
            if (f >= J.chunk_base[lo] && f < J.chunk_base[lo] + n) { *c = f - J.chunk_base[lo]; return lo; }
            if (n > 0) return -1;
        }
        lo--;
    }
    return -1;
}
template <int SEL> static __global__ void __launch_bounds__(64) k_stream_scan(const StreamJobs J)
{
    __shared__ uint32_t s_win[SI_WIN_DWORDS];
    long long c = 0;
    const int i = stream_of_chunk(J, blockIdx.x, &c);
    if (i < 0) return;
    const SiWork W = {s_win, nullptr};
    si_scan(W, J.bytes + J.off[i], J.len[i], c, 0, J.chunks + blockIdx.x, stream_table(J, i, SEL));
}
template <int SEL> static __global__ void __launch_bounds__(64) k_stream_prefix(const StreamJobs J)
{
    __shared__ SiChunk s_sc[64];
    const int i = blockIdx.x;
    if (J.bad[i]) return;
    const SiWork W = {nullptr, s_sc};
    const uint8_t *src = J.bytes + J.off[i];
    si_prefix(W, src, J.len[i], J.chunks + J.chunk_base[i], si_chunks(src, J.len[i]), stream_table(J, i, SEL), J.n_units + i, J.n_slices + i);
}
template <int SEL> static __global__ void __launch_bounds__(64) k_stream_place(const StreamJobs J)
{
    __shared__ uint32_t s_win[SI_WIN_DWORDS];
    long long c = 0;
    const int i = stream_of_chunk(J, blockIdx.x, &c);
    if (i < 0) return;
    const SiWork W = {s_win, nullptr};
    si_scan(W, J.bytes + J.off[i], J.len[i], c, 1, J.chunks + blockIdx.x, stream_table(J, i, SEL));
}

/* one step of the stream receiver: context i's next slice unit (table[i * max_units + cursor[i]], a unit of its stream bytes[soff[i] ..
 * + slen[i])) unescaped to rbsp[i * slot ..), then what the parsers read: off / len / start_bit / qp.  first[i]: the code of the first
 * stage that failed */
struct StreamStep {
    const uint8_t *bytes; long long bytes_size;
    const long long *soff, *slen; const int *bad;
    const pcamv_unit_t *table; long long max_units, stride; const long long *n_slices; long long *cursor;
    uint8_t *rbsp; long long slot, rbsp_size;       /* (the header probe: any buffer of rbsp_size bytes, off / len the caller's) */
    long long *off, *len, *start_bit; int *qp, *first, *nal_header, *frame_num;
    pcamv_stream_params_t P;
    int n;
    /* a window of k units per context (k_stream_window_unit): the job arrays hold n * k entries, context-major (job i * k + w), `n` counts
     * jobs, and cursor_was is a copy of the cursors made before the launch -- what the slot waves read, while one lane moves `cursor` */
    const long long *cursor_was; int k;
    /* k_slice_header_sets: the table of context i / sets_k, the entropy mode of the batch's contexts, and where the entry's mode goes */
    const pcamv_param_sets_t *sets; int sets_k, want_cabac; int *entropy;
};
static __global__ void __launch_bounds__(64) k_stream_unit(const StreamStep J)
{
    __shared__ uint32_t s_win[NU_WIN_DWORDS], s_out[NU_OUT_DWORDS];
    const int i = blockIdx.x, lane = threadIdx.x;
    const NuWork W = {s_win, s_out};
    const long long cur = J.cursor[i], total = J.bad[i] ? 0 : J.n_slices[i], have = total < J.max_units ? total : J.max_units;
    int rc = J.bad[i] ? PCAMV_EINVAL : PCAMV_EEOF, done = 0;      /* (a stream the index call refused has no end to be at) */
    if (cur >= 0 && cur < have) {
        const pcamv_unit_t u = J.table[(long long)i * J.stride + cur];
        const long long soff = J.soff[i], slen = J.slen[i];
        if (lane == 0) J.cursor[i] = cur + 1;
        rc = u.kind == PCAMV_UNIT_PSLICE ? PCAMV_EINVAL : PCAMV_EUNSUP;
        if (u.kind == PCAMV_UNIT_PSLICE && u.off >= 0 && u.len >= 0 && u.len <= slen && u.off <= slen - u.len && u.len <= J.slot + 1 && soff >= 0 &&
            slen <= J.bytes_size && soff <= J.bytes_size - slen) {
            rc = pcamv_nal_unescape(W, J.bytes + soff + u.off, u.len, J.rbsp + (long long)i * J.slot, J.len + i, J.nal_header + i);
            done = 1;
        }
    }
    if (lane == 0) {
        if (!done) { J.len[i] = -1; J.nal_header[i] = -1; }
        J.off[i] = (long long)i * J.slot; J.first[i] = rc; J.start_bit[i] = 0; J.qp[i] = 0; J.frame_num[i] = -1;
    }
}
/* the same for slot w of context i, job j = i * k + w of a launch of n contexts x k slots: the unit at cursor + w into the job's own RBSP
 * slot.  Slots beyond the table's end take nothing (PCAMV_EEOF); the wave of slot 0 moves the context's cursor over the slots that took
 * a unit.  No wave waits on another: every wave reads the cursor's copy, which no kernel of the launch writes */
static __global__ void __launch_bounds__(64) k_stream_window_unit(const StreamStep J)
{
    __shared__ uint32_t s_win[NU_WIN_DWORDS], s_out[NU_OUT_DWORDS];
    const int j = blockIdx.x, i = j / J.k, w = j - i * J.k, lane = threadIdx.x;
    const NuWork W = {s_win, s_out};
    const long long was = J.cursor_was[i], cur = was + w, total = J.bad[i] ? 0 : J.n_slices[i], have = total < J.max_units ? total : J.max_units;
    int rc = J.bad[i] ? PCAMV_EINVAL : PCAMV_EEOF, done = 0;
    if (was >= 0 && cur < have) {
        const pcamv_unit_t u = J.table[(long long)i * J.stride + cur];
        const long long soff = J.soff[i], slen = J.slen[i];
        rc = u.kind == PCAMV_UNIT_PSLICE ? PCAMV_EINVAL : PCAMV_EUNSUP;
        if (u.kind == PCAMV_UNIT_PSLICE && u.off >= 0 && u.len >= 0 && u.len <= slen && u.off <= slen - u.len && u.len <= J.slot + 1 && soff >= 0 &&
            slen <= J.bytes_size && soff <= J.bytes_size - slen) {
            rc = pcamv_nal_unescape(W, J.bytes + soff + u.off, u.len, J.rbsp + (long long)j * J.slot, J.len + j, J.nal_header + j);
            done = 1;
        }
    }
    if (lane == 0) {
        if (w == 0 && was >= 0 && was < have) J.cursor[i] = was + (have - was < J.k ? have - was : J.k);
        if (!done) { J.len[j] = -1; J.nal_header[j] = -1; }
        J.off[j] = (long long)j * J.slot; J.first[j] = rc; J.start_bit[j] = 0; J.qp[j] = 0; J.frame_num[j] = -1;
    }
}
/* one lane per slice: the header of RBSP i (bytes[off[i] .. + len[i]) of the buffer the parser will read) */
static __global__ void __launch_bounds__(64) k_slice_header(const StreamStep J)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= J.n || J.first[i]) return;
    const long long off = J.off[i], len = J.len[i];
    long long sb = -1; int qp = -1, fn = -1, rc = PCAMV_EINVAL;
    if (off >= 0 && len >= 0 && len <= J.rbsp_size && off <= J.rbsp_size - len) rc = pcamv_slice_header_read(J.rbsp + off, len, J.nal_header[i], J.P, &sb, &qp, &fn);
    J.start_bit[i] = sb; J.qp[i] = qp; J.frame_num[i] = fn;
    if (rc) { J.first[i] = rc; J.len[i] = -1; }         /* as the unescaper marks a unit that failed: the parser refuses it */
}
/* the same under the parameter sets of the slice's own stream: the table of context i / sets_k, the entry its pps_id names */
static __global__ void __launch_bounds__(64) k_slice_header_sets(const StreamStep J)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= J.n) return;
    J.entropy[i] = -1;
    if (J.first[i]) return;
    const long long off = J.off[i], len = J.len[i];
    long long sb = -1; int qp = -1, fn = -1, mode = -1, rc = PCAMV_EINVAL;
    if (off >= 0 && len >= 0 && len <= J.rbsp_size && off <= J.rbsp_size - len)
        rc = pcamv_slice_header_read_sets(J.rbsp + off, len, J.nal_header[i], J.sets[i / J.sets_k], J.want_cabac, &sb, &qp, &fn, &mode);
    J.start_bit[i] = sb; J.qp[i] = qp; J.frame_num[i] = fn; J.entropy[i] = mode;
    if (rc) { J.first[i] = rc; J.len[i] = -1; }
}
/* (a window, k > 0: job i is slot i % k of context i / k, and the last slot's code is also the context's own word -- what k steps leave) */
static __global__ void __launch_bounds__(64) k_stream_status(const int *__restrict__ first, int *__restrict__ status, int n, int *__restrict__ ctx_status, int k)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (first[i]) status[i] = first[i];
    if (k > 0 && i % k == k - 1) ctx_status[i / k] = status[i];
}

/* ---- parameter sets.  Stream i is bytes[soff[i] .. + slen[i]); its units of type 7 / 8 are table[i * PCAMV_PSET_UNITS_MAX ..) (the first
 * PCAMV_PSET_UNITS_MAX of count[i]).  The launch's units are numbered stream by stream: unit j is unit u_index[j] of stream u_stream[j],
 * stream i's are [u_base[i], u_base[i + 1]).  Unit j's RBSP goes to its slot of PCAMV_PSET_UNIT_BYTES bytes, its record to rec[j] */
struct PsetJobs {
    const uint8_t *bytes; long long bytes_size;
    const long long *soff, *slen; const int *bad;
    const pcamv_unit_t *table; const long long *count;
    const int *u_stream, *u_index; const long long *u_base; int n_units;
    uint8_t *slots; long long *rbsp_len; int *nal_header, *first; PsRec *rec;
    pcamv_param_sets_t *sets; int n, want_w, want_h;
};
/* one wavefront per unit: the unescaper of k_nal_to_rbsp into the unit's slot */
static __global__ void __launch_bounds__(64) k_pset_unit(const PsetJobs J)
{
    __shared__ uint32_t s_win[NU_WIN_DWORDS], s_out[NU_OUT_DWORDS];
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= J.n_units) return;
    const NuWork W = {s_win, s_out};
    const int i = J.u_stream[j], x = J.u_index[j];
    int rc = PCAMV_EINVAL, done = 0;
    if (i >= 0 && i < J.n && x >= 0 && x < PCAMV_PSET_UNITS_MAX && !J.bad[i]) {
        const pcamv_unit_t u = J.table[(long long)i * PCAMV_PSET_UNITS_MAX + x];
        const long long soff = J.soff[i], slen = J.slen[i];
        if (u.off >= 0 && u.len >= 1 && u.len <= slen && u.off <= slen - u.len && soff >= 0 && slen <= J.bytes_size && soff <= J.bytes_size - slen) {
            if (u.len > PCAMV_PSET_UNIT_BYTES) { rc = PCAMV_EUNSUP; if (lane == 0) J.nal_header[j] = u.nal_header; }
            else rc = pcamv_nal_unescape(W, J.bytes + soff + u.off, u.len, J.slots + (long long)j * PCAMV_PSET_UNIT_BYTES, J.rbsp_len + j, J.nal_header + j);
            done = 1;
        }
    }
    if (lane == 0) {
        if (!done) J.nal_header[j] = -1;
        if (rc) J.rbsp_len[j] = -1;
        J.first[j] = rc;
    }
}
/* one lane per unit: the RBSP parsed into the unit's record; a unit that failed before keeps its code */
static __global__ void __launch_bounds__(64) k_pset_parse(const PsetJobs J)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= J.n_units) return;
    const long long len = J.rbsp_len[j];
    const int hdr = J.nal_header[j];
    if (J.first[j] || len < 0 || len > PCAMV_PSET_UNIT_BYTES) {
        PsRec r;
        memset(&r, 0, sizeof(r));
        r.code = J.first[j] ? J.first[j] : PCAMV_EINVAL; r.type = hdr < 0 ? 0 : hdr & 31;
        J.rec[j] = r;
        return;
    }
    ps_parse_unit(J.slots + (long long)j * PCAMV_PSET_UNIT_BYTES, len, hdr, J.rec + j);
}
/* one wavefront per stream: its records resolved into its table */
static __global__ void __launch_bounds__(64) k_pset_resolve(const PsetJobs J)
{
    const int i = blockIdx.x;
    if (i >= J.n) return;
    const long long base = J.u_base[i], have = J.u_base[i + 1] - base;
    long long count = J.bad[i] ? 0 : J.count[i];
    if (count < have) count = have;             /* (never: the host listed min(count, PCAMV_PSET_UNITS_MAX) of them) */
    ps_resolve(J.rec + base, have < PCAMV_PSET_UNITS_MAX ? have : count, J.bad[i] ? PCAMV_EINVAL : 0, J.want_w, J.want_h, J.sets + i);
}

/* ---- the sender's byte streams (pcamv_stream_write.h), one lane per context.  ctx, table, slot, w_len are the library's; bytes and len
 * the caller's (stream_open).  table is the header table the slice writer reads (WriteJobs::hdr, n entries), slot / w_len / status what
 * it reads as off, cap and writes as len, status */
static_assert(SWS_HDR_WORDS == SW_HDR_WORDS, "k_stream_slot writes the table the slice writers read");
struct StreamWrite {
    uint8_t *bytes; long long bytes_size;
    SwsCtx *ctx; int *table;
    long long *w_off, *w_cap, *w_len, *len; int *first, *status;
    const long long *off, *cap; const uint8_t *head; long long head_len;       /* k_stream_open alone */
    SwsSetup S;
    int n;
};
static __global__ void __launch_bounds__(64) k_stream_open(const StreamWrite J)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= J.n) return;
    SwsCtx c;
    long long len = 0;
    sws_open(c, J.bytes, J.bytes_size, J.off[i], J.cap[i], J.head, J.head_len, &len);
    J.ctx[i] = c; J.len[i] = len;
}
static __global__ void __launch_bounds__(64) k_stream_slot(const FrameDev *__restrict__ Fs, const StreamWrite J)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= J.n) return;
    const SwsSlot s = sws_slot(J.S, J.ctx[i], J.bytes, Fs[i].qp, J.table, J.n, i);
    J.w_off[i] = s.off; J.w_cap[i] = s.cap; J.first[i] = s.first;
}
static __global__ void __launch_bounds__(64) k_stream_commit(const StreamWrite J)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= J.n) return;
    SwsCtx c = J.ctx[i];
    long long len = 0; int rc = 0;
    sws_commit(J.S, c, J.first[i], J.w_len[i], J.status[i], &len, &rc);
    J.ctx[i] = c; J.len[i] = len; J.status[i] = rc;
}
/* ---- one video of many chains (pcamv_video.h).  A copy launch: n jobs of offsets into src and dst, made by the kernel in front of it;
 * chunk_base[0 .. n] is k_stream_copy_plan's.  The grid is sized by what the host knows the jobs cannot exceed, and capped: a wavefront
 * takes flat chunks blockIdx.x, blockIdx.x + gridDim.x, ... below the total the plan found, and none if there is none for it */
struct CopyJobs { const uint8_t *src; uint8_t *dst; VcJob *jobs; long long *chunk_base; int n; };
static __global__ void __launch_bounds__(64) k_stream_copy_plan(const CopyJobs J)
{
    __shared__ long long s_sum[64];
    vc_plan(s_sum, J.dst, J.jobs, J.n, J.chunk_base);
}
static __global__ void __launch_bounds__(64) k_stream_copy(const CopyJobs J)
{
    const long long total = J.chunk_base[J.n];
    for (long long f = blockIdx.x; f < total; f += gridDim.x) {
        long long c = 0;
        const VcJob j = J.jobs[vc_job_of(J.chunk_base, J.n, f, &c)];
        vc_copy_chunk(J.src + j.src, J.dst + j.dst, j.len, c);
    }
}
/* stream_open with a head per context: one lane per context decides and makes the context's copy job (J.head: the heads' buffer) */
struct HeadJobs { long long heads_size; const long long *head_off, *head_len; VcJob *jobs; };
static __global__ void __launch_bounds__(64) k_stream_open_heads(const StreamWrite J, const HeadJobs H)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= J.n) return;
    SwsCtx c;
    long long len = 0;
    H.jobs[i] = vj_head(c, J.bytes_size, J.off[i], J.cap[i], H.heads_size, H.head_off[i], H.head_len[i], &len);
    J.ctx[i] = c; J.len[i] = len;
}
struct JoinJobs { const SwsCtx *ctx; int n; long long video_size; const long long *video_off; long long *video_len, *placed; int *status; VcJob *jobs; };
static __global__ void __launch_bounds__(64) k_stream_join(const JoinJobs J)
{
    __shared__ long long s_sum[64];
    vj_join(s_sum, J.ctx, J.n, J.video_size, J.video_off, J.video_len, J.placed, J.status, J.jobs);
}
/* one wavefront per video: video v's units are table[v * stride .. + n_units[v]) (all of them: the index kernels were given room for the
 * count), its GOPs go to gops[v * gstride ..) and, for the one video of a batch, to the contexts' (off, len).  A video the index refused
 * has PCAMV_EINVAL for both counts */
struct VideoCut {
    const pcamv_unit_t *table; long long stride; const long long *n_units, *off, *len; const int *bad;
    pcamv_gop_t *gops; long long gstride, first, cap;
    long long *ctx_off, *ctx_len; int n_ctx;
    long long *n_gops, *preamble;
};
static __global__ void __launch_bounds__(64) k_video_cut(const VideoCut J)
{
    __shared__ long long s_start[65], s_unit[65];
    const int v = blockIdx.x;
    if (J.bad[v]) {
        if (threadIdx.x == 0) { J.n_gops[v] = PCAMV_EINVAL; J.preamble[v] = PCAMV_EINVAL; }
        for (int r = threadIdx.x; r < J.n_ctx; r += 64) { J.ctx_off[r] = 0; J.ctx_len[r] = 0; }
        return;
    }
    const VgWork W = {s_start, s_unit};
    const VgOut O = {J.gops + (long long)v * J.gstride, J.first, J.cap, J.ctx_off, J.ctx_len, J.off[v], J.n_ctx, J.n_gops + v, J.preamble + v};
    long long m = J.n_units[v];
    if (m > J.stride) m = J.stride;             /* (never: the table was sized by this count) */
    vg_cut(W, J.table + (long long)v * J.stride, m, J.len[v], O);
}
/* k_stream_prefix for an index of ONE stream, in two levels (vp_local / si_prefix over the blocks / vp_apply): B has room for a summary
 * per VP_BLOCK chunks.  The grids are sized by max_chunks; what lies beyond the stream's chunks exits */
static __global__ void __launch_bounds__(64) k_video_prefix_local(const StreamJobs J, SiChunk *__restrict__ B)
{
    __shared__ SiChunk s_sc[64];
    if (J.bad[0]) return;
    const uint8_t *src = J.bytes + J.off[0];
    const long long n_chunks = si_chunks(src, J.len[0]);
    if ((long long)blockIdx.x * VP_BLOCK >= n_chunks) return;
    const SiWork W = {nullptr, s_sc};
    vp_local(W, src, J.len[0], J.chunks + J.chunk_base[0], n_chunks, blockIdx.x, B);
}
template <int SEL> static __global__ void __launch_bounds__(64) k_video_prefix_top(const StreamJobs J, SiChunk *__restrict__ B)
{
    __shared__ SiChunk s_sc[64];
    if (J.bad[0]) return;
    const uint8_t *src = J.bytes + J.off[0];
    const SiWork W = {nullptr, s_sc};
    si_prefix(W, src, J.len[0], B, (si_chunks(src, J.len[0]) + VP_BLOCK - 1) / VP_BLOCK, stream_table(J, 0, SEL), J.n_units, J.n_slices);
}
static __global__ void __launch_bounds__(64) k_video_prefix_apply(const StreamJobs J, const SiChunk *__restrict__ B)
{
    if (J.bad[0]) return;
    vp_apply(J.chunks + J.chunk_base[0], si_chunks(J.bytes + J.off[0], J.len[0]), B, (long long)blockIdx.x * 64 + threadIdx.x);
}
/* the video's one table of parameter sets to every context */
static __global__ void __launch_bounds__(64) k_pset_spread(const pcamv_param_sets_t *__restrict__ one, pcamv_param_sets_t *__restrict__ sets, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) sets[i] = *one;
}
/* the parity probe of the header writer: case i's parameter set and members, its slot of PCAMV_SLICE_HDR_BYTES bytes (zeros beforehand) */
static __global__ void __launch_bounds__(64) k_slice_headers_write(const pcamv_stream_params_t *__restrict__ P, const pcamv_slice_fields_t *__restrict__ f,
                                                                   int n, int *__restrict__ rc, int *__restrict__ n_bits, uint8_t *__restrict__ bits)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int nb = 0;
    rc[i] = pcamv_slice_header_write(P[i], f[i], bits + (long long)i * PCAMV_SLICE_HDR_BYTES, &nb);
    n_bits[i] = nb;
}
/* the writer's kernel is a unit of its own (pcamv_slice_write.hip): it inlines the analysis' prediction and transform primitives, and what
 * the compiler makes of the kernels of this unit depends on what else in the unit calls them */
void pcamv_launch_write_pslice(unsigned slices, hipStream_t st, const FrameDev *dF, const WriteJobs &J);
void pcamv_launch_write_pslice_cavlc(unsigned slices, hipStream_t st, const FrameDev *dF, const WriteJobs &J);   /* pcamv_slice_write_cavlc.hip */
#endif
