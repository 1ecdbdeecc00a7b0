/*
 * pcamv_gpu.hip -- host side of libpcamv_gpu.so: the C ABI of include/pcamv_gpu.h over the
 * gfx950 kernels of pcamv_planes.hip.h, pcamv_kernels.hip.h and pcamv_embed.hip.h, which this unit alone compiles, and the launchers
 * of the other instances of the analysis kernel (pcamv_flow.hip.h).  There is no CPU path: every entry point needs a HIP
 * device and fails with PCAMV_ENODEV / PCAMV_EHIP otherwise.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "pcamv_planes.hip.h"
#include "pcamv_kernels.hip.h"
#include "pcamv_embed.hip.h"
#include "pcamv_message.hip.h"
#include "pcamv_slice.hip.h"
#include "pcamv_rate.hip.h"
#include "pcamv_source.hip.h"
#include "pcamv_host_tables.h"
#include "pcamv_mvsyntax.h"
#include "pcamv_param_sets_host.h"
#include "pcamv_rd_select.h"
#include "pcamv_idr_defs.h"

#define PCAMV_ABI_VERSION 3
#define NEV 32                 /* launches the analysis kernel's timer remembers between two kernel_time calls ... */
#define NRING 8
#define NKEV 16                /* ... and a timer of the smaller kernels */
/* The timed kernels, stated here only: X(timer, the name pcamv_gpu_batch_kernel_time knows it by); the enum and the table of names
 * (kt_name) are made from the list, so a timer has its place in both or in neither.  KT_ANALYSE goes by the name of the batch's
 * instance of the analysis kernel (dominant_kernel) */
#define PCAMV_TIMERS(X) \
    X(KT_ANALYSE, NULL) \
    X(KT_EMBED_PREPARE, "k_embed_prepare") X(KT_EXTRACT_PREPARE, "k_extract_prepare") X(KT_EXTRACT_BITS, "k_extract_bits") \
    X(KT_PAYLOAD_CHECK, "k_payload_check") X(KT_PARSE_PSLICE, "k_parse_pslice") X(KT_PARSE_PSLICE_CAVLC, "k_parse_pslice_cavlc") \
    X(KT_WRITE_PSLICE, "k_write_pslice") X(KT_WRITE_PSLICE_CAVLC, "k_write_pslice_cavlc") X(KT_NAL_TO_RBSP, "k_nal_to_rbsp") \
    X(KT_STREAM_PLAN, "k_stream_plan") X(KT_STREAM_SCAN, "k_stream_scan") X(KT_STREAM_PREFIX, "k_stream_prefix") \
    X(KT_STREAM_PLACE, "k_stream_place") X(KT_STREAM_UNIT, "k_stream_unit") X(KT_SLICE_HEADER, "k_slice_header") \
    X(KT_STREAM_STATUS, "k_stream_status") X(KT_STREAM_OPEN, "k_stream_open") X(KT_STREAM_SLOT, "k_stream_slot") \
    X(KT_STREAM_COMMIT, "k_stream_commit") X(KT_STREAM_WINDOW_UNIT, "k_stream_window_unit") X(KT_EXTRACT_COUNT, "k_extract_count") \
    X(KT_EXTRACT_CHAIN, "k_extract_chain") X(KT_PSET_UNIT, "k_pset_unit") X(KT_PSET_PARSE, "k_pset_parse") \
    X(KT_PSET_RESOLVE, "k_pset_resolve") X(KT_SLICE_HEADER_SETS, "k_slice_header_sets") X(KT_STREAM_OPEN_HEADS, "k_stream_open_heads") \
    X(KT_STREAM_JOIN, "k_stream_join") X(KT_STREAM_COPY_PLAN, "k_stream_copy_plan") X(KT_STREAM_COPY, "k_stream_copy") \
    X(KT_VIDEO_CUT, "k_video_cut") X(KT_MESSAGE_COUNT, "k_message_count") X(KT_MESSAGE_PLAN, "k_message_plan") \
    X(KT_MESSAGE_JOBS, "k_message_jobs") X(KT_EXTRACT_CHAIN_MESSAGE, "k_extract_chain_message") X(KT_MESSAGE_CHECK, "k_message_check") \
    X(KT_IDR_MB, "k_idr_mb") X(KT_IDR_PREFIX, "k_idr_prefix") X(KT_IDR_PACK, "k_idr_pack") X(KT_IDR_UNIT, "k_idr_unit") \
    X(KT_IDR_DEBLOCK, "k_idr_deblock") X(KT_IDR_UNIT_LEN, "k_idr_unit_len") X(KT_IDR_PLACE, "k_idr_place") X(KT_IDR_MB4, "k_idr_mb4") \
    X(KT_FRAME_QP, "k_frame_qp") X(KT_RATE_UPDATE, "k_rate_update") X(KT_SOURCE_FEED, "k_source_feed")
#define KT_ENUM(id, name) id,
enum { PCAMV_TIMERS(KT_ENUM) KT_N };
#undef KT_ENUM
#define PCAMV_FEATURES (PCAMV_FEATURE_PAYLOAD | PCAMV_FEATURE_SLICE_PARSER | PCAMV_FEATURE_SLICE_PARSER_CAVLC | PCAMV_FEATURE_SLICE_WRITER | \
                        PCAMV_FEATURE_SLICE_WRITER_CAVLC | PCAMV_FEATURE_NAL_DEVICE | PCAMV_FEATURE_STREAM_DEVICE | PCAMV_FEATURE_STREAM_WRITER | \
                        PCAMV_FEATURE_STREAM_WINDOW | PCAMV_FEATURE_PARAM_SETS | PCAMV_FEATURE_VIDEO | PCAMV_FEATURE_MESSAGE | PCAMV_FEATURE_IDR | \
                        PCAMV_FEATURE_IDR_DEBLOCK | PCAMV_FEATURE_IDR_SLICES | PCAMV_FEATURE_IDR_I4X4 | PCAMV_FEATURE_RATE | PCAMV_FEATURE_SOURCE)
#define SRC_GUARD_BYTE 0xC3     /* what the PCAMV_SRC_GUARD bytes behind a context's source planes hold */
#define MSG_GUARD_WORDS 4       /* words behind a batch's received stream that nothing may write */
#define SLICE_GUARD_MBS 4       /* records behind a context's receive-side records that nothing may write (pcamv_gpu_debug_slice_records) */
#define NSTAGE 2                /* staging buffers of extract_slices: a call waits for the one before the last */
/* the stages of a step (batch_launch's `what`): plane production, analysis (search + RCA + encode), embedding, second pass */
enum { ST_PLANES = 1, ST_ANALYSE = 2, ST_EMBED = 4, ST_PASS2 = 8 };

/* what device code assumes of constants it cannot see side by side (this unit includes both headers) */
static_assert(sizeof(pcamv_mb_t) == 59 * 4, "p2_unit_load copies a record as 59 dwords: a field added to pcamv_mb_t truncates or misaligns the second pass' LDS copy");
static_assert(4 * P2_LROW(8) <= P2_TW && 4 * P2_CROW(8) <= P2_CW, "a tile row of the longest run (8 macroblocks and the four columns left of it) no longer fits the tile's pitch");
static_assert(FLOW_SPEC_MIN_MBW - 1 > FLOW_SPEC_AHEAD + 1, "speculative chain: a macroblock would be handed on before its top / top-right neighbours are final");

/* The builds of the RD instance of the analysis kernel (one translation unit each, pcamv_rd.hip), a row per entry of
 * PCAMV_RD_BUILDS in the order of rd_select's result; the phase timers are per translation unit (PCAMV_PROF) */
struct RdBuild {
    int spec;                   /* waves per SIMD of the speculative raster chain, 0: plain chain */
    void (*launch)(unsigned waves, hipStream_t st, const FrameDev *dF, const FlowDev &fl);
    int (*waves_per_cu)(void);
    int (*prof_fetch)(unsigned long long *out, int reset);      /* NULL without PCAMV_PROF */
};
#ifdef PCAMV_PROF
#define RD_PROF_FN(id) pcamv_rd_prof_fetch<RD_##id>
#else
#define RD_PROF_FN(id) NULL
#endif
#define RD_ROW(id, occ, variant) {rd_build_spec(RD_##id), pcamv_launch_flow_rd<RD_##id>, pcamv_flow_rd_waves_per_cu<RD_##id>, RD_PROF_FN(id)},
static const RdBuild rd_builds[RD_N_BUILDS] = {PCAMV_RD_BUILDS(RD_ROW)};

/* the error text of a context or of a batch */
template <class Owner> static int fail(Owner *o, int code, const char *fmt, ...)
{
    if (o) { va_list ap; va_start(ap, fmt); vsnprintf(o->err, sizeof(o->err), fmt, ap); va_end(ap); }
    return code;
}
#define HIPCHK(o, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(o, PCAMV_EHIP, "%s: %s", #call, hipGetErrorString(e_)); } while (0)
#define TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

template <class T> static hipError_t dalloc(T **p, size_t n) { return hipMalloc((void **)p, n * sizeof(T)); }
/* Memory with one owner -- a batch or one of its parts, or the scope of a call -- which frees it when it goes: `cap` elements on the
 * device (DevBuf), or in pinned host memory (PinBuf).  Pointers into somebody else's memory stay plain pointers.
 * room() grows it and never shrinks it.  Freeing waits for the device, so a room() that may grow belongs in calls that may wait: creation,
 * index calls, stream_window, stream_param_sets, set_message, the reserve calls, the opens and idr_setup behind their synchronisation,
 * probes.  On the paths that queue work and return (steps, extract calls, write calls) it stands only where it finds its room, or
 * makes it once for good (a batch's first extraction, a staging buffer outgrown: stage_take) */
template <class T, bool PINNED = false> struct DevBuf {
    T *p = NULL; size_t cap = 0;
    DevBuf() = default; DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete; ~DevBuf() { release(); }
    void release() { if (p) PINNED ? hipHostFree(p) : hipFree(p); p = NULL; cap = 0; }
    /* oom: the owner's code for a device without memory left */
    template <class Owner> int room(Owner *o, size_t n, int oom = PCAMV_EHIP)
    {
        if (p && n <= cap) return 0;
        release();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p, (n ? n : 1) * sizeof(T), hipHostMallocDefault) : dalloc(&p, n ? n : 1);
        if (e != hipSuccess) return fail(o, e == hipErrorOutOfMemory ? oom : PCAMV_EHIP, "%zu bytes of %s memory: %s", n * sizeof(T), PINNED ? "pinned host" : "device", hipGetErrorString(e));
        cap = n;
        return 0;
    }
    operator T *() const { return p; }
};
template <class T> using PinBuf = DevBuf<T, true>;

/* a ring of N slots taken in turn (ring_take, ring_release): a slot is written again only after the work that read it last (its event,
 * made when the slot is first taken) is done */
template <int N> struct EvRing {
    int head = 0, used[N] = {}; hipEvent_t done[N] = {};
    EvRing() = default; EvRing(const EvRing &) = delete;
    ~EvRing() { for (hipEvent_t e : done) if (e) hipEventDestroy(e); }
};
/* hipEvents around the launches of one kernel, summed when pcamv_gpu_batch_kernel_time asks for it by name: a ring of the last `cap`
 * launches; one pair of events stands for `weight` launches (the anti-diagonals of PCAMV_SCHED=diag share a pair) */
struct KTimer {
    hipEvent_t e0[NEV], e1[NEV]; int cap, weight, made, n, head, launches; double ms;
    ~KTimer() { for (int i = 0; i < NEV; i++) { if (e0[i]) hipEventDestroy(e0[i]); if (e1[i]) hipEventDestroy(e1[i]); } }
};
/* NSTAGE staging buffers taken in turn, each a pinned host block and its device copy made by the calls themselves (stage_take): a buffer
 * is filled again only after the work that read it last (its event) is done, so a call waits for the one before the last.  A ring
 * that only kernels fill (nal_stage, su_stage) has no host blocks */
struct StageRing { EvRing<NSTAGE> ring; PinBuf<uint8_t> h[NSTAGE]; DevBuf<uint8_t> d[NSTAGE]; };

/* the index of n byte streams (k_stream_plan .. k_stream_place): the library's copy of their placement, the working memory of the
 * scan, the tables; for a batch also what its steps need -- the borrowed buffer and the size of an RBSP slot */
struct StreamIndex {
    int n, ready;
    long long max_units, stride, max_chunks;
    DevBuf<long long> d_at;     /* [off n][len n][chunk_base n][n_units n][n_slices n][cursor n] */
    DevBuf<int> d_bad; DevBuf<unsigned long long> d_longest; DevBuf<SiChunk> d_chunks; DevBuf<pcamv_unit_t> d_table; DevBuf<uint8_t> d_own;
    const uint8_t *bytes; long long bytes_size, slot;       /* (borrowed: the caller's buffer, or d_own) */
    DevBuf<SiChunk> d_keep;     /* a video's index (video_units_run): the chunks' summaries as the first scan left them */
};

/* the parameter sets of n indexed streams (k_pset_unit, k_pset_parse, k_pset_resolve): the tables of their units of type 7 / 8, the
 * per-stream counts, and per unit of the last run its place, slot and record; d_sets is what k_slice_header_sets reads.  `ready` holds
 * from a stream_param_sets call to the next index call */
struct StreamSets {
    int ready;
    DevBuf<pcamv_unit_t> d_table; DevBuf<long long> d_cnt; DevBuf<pcamv_param_sets_t> d_sets;   /* d_cnt: [n_units n][count n][u_base n + 1] */
    DevBuf<long long> d_len; DevBuf<int> d_map; DevBuf<PsRec> d_rec; DevBuf<uint8_t> d_slots;  /* d_map: [u_stream U][u_index U][nal_header U][first U] */
};

/* the byte streams a batch writes (pcamv_gpu_batch_stream_open): the borrowed buffer and length array, the settings every picture shares,
 * and in one block of the library's per context the stream's state, the header table the slice writer reads, and what passes between
 * k_stream_slot, the writer and k_stream_commit */
struct StreamOut {
    int ready;
    uint8_t *bytes; long long bytes_size; long long *len;       /* (borrowed: the caller's) */
    SwsSetup S;
    DevBuf<uint8_t> d_own;              /* [SwsCtx n][w_off n][w_cap n][w_len n][off n][cap n][first n][table: n entries, n slots] */
    DevBuf<uint8_t> d_head;
    DevBuf<uint8_t> d_copy;             /* the copy launches of stream_open_heads and join_streams: [VcJob n][chunk_base n + 1][head_off n][head_len n][join status] */
    int joined;                         /* a join was queued since the open: its status is there to be read */
    int stepped;                        /* a write_stream_step or a write_stream_idr was queued since the open: an IDR picture no longer belongs here */
};

/* the slots of a window of slice units per context (pcamv_gpu_batch_stream_window): per context x slot what a step keeps per context --
 * receive-side records with their guard, stego, hdr, cols, a status word, a row-scratch slot for wide pictures -- then the job arrays and
 * RBSP slots of n * k jobs in one block, the copy of the cursors a launch reads, and NSTAGE sets of n * k descriptors taken in turn.
 * Job i * k_call + w of a call is slot w of context i, and that job's memory is entry i * k_call + w of every array here */
struct StreamWindow {
    int k, k_last;              /* slots reserved per context; slots of the last window call */
    DevBuf<pcamv_mb_t> d_mbs; DevBuf<uint8_t> d_stego; DevBuf<int> d_hdr; DevBuf<unsigned> d_cols; DevBuf<int> d_stat; DevBuf<uint8_t> d_scratch;
    DevBuf<uint8_t> d_jobs;
    DevBuf<long long> d_cursor_was;
    PinBuf<ExtractDev> h_X; DevBuf<ExtractDev> d_X; EvRing<NSTAGE> desc;
    hipEvent_t done; int used;  /* behind the last window call: the next one's stream waits for it, since they share the slots */
    ~StreamWindow() { if (done) hipEventDestroy(done); }
};

struct pcamv_ctx;
/* A batch = the set of independent closed-GOP contexts whose frames advance together: every kernel
 * launch carries the same dependency step of all of them (descriptor arrays in device memory). */
struct pcamv_batch {
    int n, device, n_diag, slots_per_mb, max_diag;
    int W, H;
    pcamv_ctx **ctx;
    PinBuf<FrameDev> h_F; DevBuf<FrameDev> d_F;         /* NRING slots of n descriptors (pinned host / device) */
    PinBuf<EmbedDev> h_E; DevBuf<EmbedDev> d_E;
    EvRing<NRING> ring;
    /* dataflow schedule (k_analyse_flow): queue + dependency counters, one persistent launch per step */
    int sched_flow, flow_waves, flow2_waves, closed_loop, stc_ns;
    int b_mbrd, b_tesa;         /* instance of the analysis kernel the batch's contexts need (fixed at creation) */
    const RdBuild *rd;          /* ... and which build of the RD instance (b_mbrd) */
    DevBuf<unsigned> d_flow;
    FlowDev fl, fl2;          /* queue descriptors of the analysis and of the second pass (pointers into d_flow) */
    /* payload path: descriptors of the receiving side (their own ring, made by the first extraction) and the per-context counts of
     * payload_check */
    PinBuf<ExtractDev> h_X; DevBuf<ExtractDev> d_X; DevBuf<long long> d_chk;
    EvRing<NRING> xring;
    /* receiver from a stream (k_parse_pslice, k_parse_pslice_cavlc; a batch is of one entropy mode): per-context status words, the tables, the row buffers of pictures too wide for LDS, and
     * the staging of host slices -- descriptor arrays then bytes in one block */
    DevBuf<int> d_sstat; DevBuf<uint8_t> d_sp_tab, d_sp_scratch;
    int sp_lds_cols;            /* pictures up to this many macroblocks wide keep the parser's row buffer in LDS (SP_LDS_COLS; PCAMV_SLICE_LDS_COLS lowers it) */
    StageRing rx_stage;
    /* ... handed NAL units (k_nal_to_rbsp): the RBSPs, their lengths and header bytes, which the parser of the same call reads */
    StageRing nal_stage;
    /* ... handed byte streams: the index of every context's stream, and the job arrays and RBSP slots of a step, sized by index calls */
    StreamIndex sx;
    StreamSets ps;              /* ... and their parameter sets, for the *_sets calls */
    /* ... handed one video (pcamv_gpu_batch_index_video*): the index of the video as one stream with all its units listed, the contexts'
     * (off, len) k_video_cut makes of it -- [off n][len n][n_gops][preamble] --, and the video's own sets; `video` holds from such a call to
     * the next index call of either kind */
    StreamIndex vx; StreamSets vps; DevBuf<long long> d_vcut; int video;
    StageRing su_stage;
    StreamWindow sw;
    /* sender to a stream (k_write_pslice, k_write_pslice_cavlc): the same of its own, and the staging of the callers' slice headers -- a
     * ring apart from the receiver's, since a write and a parse of one batch may be in flight on different streams */
    DevBuf<int> d_wstat; DevBuf<uint8_t> d_sw_tab, d_sw_scratch;
    StageRing tx_stage;
    /* ... that writes byte streams (k_stream_open, k_stream_slot, k_stream_commit): what stream_open was given and the library's own of it */
    StreamOut so;
    /* one message for the batch (pcamv_message.hip.h).  Sender: the attached message (own copy, or the caller's device buffer), the state
     * words (MSG_*) with the batch cursor, and per context of a step its m and its planned place.  Receiver: the batch's received stream
     * and its state, per job of a call (m, status) and the planned place -- room for a window of PCAMV_STREAM_WINDOW_MAX --, and the
     * partial sums of message_check, the result behind them */
    const uint8_t *d_msg; long long msg_bits; DevBuf<uint8_t> d_msg_own;       /* (d_msg is borrowed: d_msg_own, or the caller's) */
    DevBuf<long long> d_mtx; DevBuf<int> d_mtx_m; DevBuf<long long> d_mtx_at;
    DevBuf<unsigned> d_mrx; long long mrx_bits; DevBuf<long long> d_mrx_state; DevBuf<int> d_mrx_job; DevBuf<long long> d_mrx_at, d_mchk;
    /* IDR pictures coded on the device (pcamv_idr.hip): the working memory of a group of `group` contexts in one block -- per place the
     * counts, the bit-string slots, the bit counts, the prefix and the RBSP --, per context a failure word, the slot's code and the probe's
     * {off, cap, len}, and the code tables */
    DevBuf<uint8_t> d_idr; int idr_group; DevBuf<uint8_t> d_idr_ctx, d_idr_tab;
    /* a QP per context on the device (pcamv_rate.h), made by the batch's first device-QP step: the MV cost tables and the slice-start
     * context states of the QPs allowed so far (qp_lo .. qp_hi), which its contexts share; a table of 52 rows per distinct (chroma offset, deadzones) among them, and
     * which of these each context reads; NRING slots of n patch jobs beside the descriptors'; the caller's array during such a step */
    DevBuf<int16_t> d_qp_cost; DevBuf<uint8_t> d_qp_cabac; DevBuf<uint32_t> d_qp_rows; std::vector<int> qp_table_of; int qp_lo, qp_hi;
    PinBuf<QpJob> h_Q; DevBuf<QpJob> d_Q;
    const int *qp_src;
    /* the rate controller: its parameters, per context its state and the cell step_rate hands to the step */
    int rate_open; pcamv_rate_params_t rate; DevBuf<pcamv_rate_state_t> d_rate; DevBuf<int> d_rate_qp;
    /* the source feed (pcamv_source.h), made by the batch's first feed: the addresses of its contexts' source planes, [n][3], and a
     * status word per context */
    DevBuf<uint8_t *> d_src_planes; DevBuf<int> d_src_status;
    KTimer kt[KT_N];            /* the timed kernels; the events of a timer are made by its first launch */
    char err[256];
};

#define CTX_NBUF 168            /* device buffers a context can own: the two per-QP tables of 52 and the ~55 buffers with a name */
struct pcamv_ctx {
    pcamv_params_t p;
    int device;
    hipStream_t stream;
    pcamv_batch *self;          /* batch of one, used by the per-context entry points */
    pcamv_batch *last;          /* batch that ran this context's most recent analysis */
    FrameDev F;
    EmbedDev E;
    /* device memory: every buffer is one hipMalloc of ctx_alloc, which notes it here for pcamv_gpu_close.  Most live in the member of
     * F / E / X that the kernels read; a field below is what such a member is pointed at and away from while the context lives */
    void *owned[CTX_NBUF]; int n_owned;
    uint8_t *d_fenc[3], *d_raw[3];
    int8_t *d_ref8, *d_prev_ref, *d_ref8_b;
    int16_t *d_mv, *d_prev_mv, *d_mv_b;
    int last_field, prev_internal;   /* ping-pong of the motion field for device-resident chains: which of d_mv (0) / d_mv_b (1) the last analysis wrote */
    pcamv_batch *member_of[16]; int n_member;    /* batches this context belongs to (its own included): told when it closes */
    int16_t *d_cost_mv[52];
    uint8_t *d_user_msg;
    int8_t *d_flip;
    int cap;
    /* payload path: the attached payload (own copy, or the caller's device buffer), the received stream and the receiver's scratch (made
     * by pcamv_gpu_rx_reserve / the first extraction); the cursors (PST_*) are E.pstate */
    uint8_t *d_payload_own; size_t payload_own_bytes;
    ExtractDev X; unsigned *d_rx; uint8_t *d_rx_bits; pcamv_mb_t *d_rx_mbs;
    pcamv_batch *win; int win_i;    /* the batch whose window call parsed this context's last slices, and the context's place in it (else NULL) */
    int *d_trace;
    int8_t *d_flip_user;       /* pass 2 */
    uint8_t *d_mbflip;         /* [n_mb] per macroblock: a carrier of it is flipped in d_flip */
    int rec_pristine;          /* F.rec / F.nnz hold the first pass' reconstruction of the frame last analysed (no second pass has run over it) */
    /* --subme >= 6 */
    uint8_t *d_cabac_init[52]; uint32_t *d_dbg_hash;
    /* the QP in force on the device: the cell {qp, status of the step that set it}; while qp_rows is set, every push of this context's
     * descriptor is patched from that table, which is qp_owner's */
    int *d_qp_cell; const uint32_t *qp_rows; pcamv_batch *qp_owner;
    char err[256];
};

/* behind the launches of an entry point: did the runtime take them all? */
template <class Owner> static int launched(Owner *o)
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail(o, PCAMV_EHIP, "kernel launch: %s", hipGetErrorString(e)) : 0;
}
/* rc of a call the batch made on behalf of context c: its error text becomes the context's */
static int on_behalf(pcamv_ctx *c, const pcamv_batch *b, int rc)
{
    if (rc) snprintf(c->err, sizeof(c->err), "%s", b->err);
    return rc;
}
/* a batch can run only while all its contexts are open */
static int batch_live(pcamv_batch *b)
{
    for (int i = 0; i < b->n; i++) if (!b->ctx[i]) return fail(b, PCAMV_EINVAL, "context %d of the batch was closed", i);
    return 0;
}

extern "C" int pcamv_gpu_abi_version(void) { return PCAMV_ABI_VERSION; }
extern "C" unsigned pcamv_gpu_features(void) { return PCAMV_FEATURES; }
#ifdef PCAMV_PROF
extern "C" int pcamv_gpu_prof_fetch(unsigned long long *out, int reset)
{
    unsigned long long rd[PCAMV_PROF_N];
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pcamv_prof), sizeof(unsigned long long) * PCAMV_PROF_N) != hipSuccess) return -1;
    if (reset) { unsigned long long z[PCAMV_PROF_N] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(pcamv_prof), z, sizeof(z)) != hipSuccess) return -1; }
    for (const RdBuild &r : rd_builds) {
        if (r.prof_fetch(rd, reset)) return -1;
        for (int i = 0; i < PCAMV_PROF_N; i++) out[i] += rd[i];
    }
    return 0;
}
#endif
extern "C" const char *pcamv_gpu_last_error(const pcamv_ctx_t *c) { return c ? c->err : "no context"; }

/* device memory of a context: `count` elements in one allocation of its own, every byte set to `fill` if that is >= 0; released by
 * pcamv_gpu_close, whichever way the context got there, or before that by ctx_free */
template <class T> static int ctx_alloc(pcamv_ctx *c, T **p, size_t count, int fill = -1)
{
    if (c->n_owned >= CTX_NBUF) return fail(c, PCAMV_ENOMEM, "a context owns at most %d device buffers", CTX_NBUF);
    HIPCHK(c, dalloc(p, count));
    c->owned[c->n_owned++] = (void *)*p;
    if (fill >= 0) HIPCHK(c, hipMemset((void *)*p, fill, count * sizeof(T)));
    return 0;
}
template <class T> static void ctx_free(pcamv_ctx *c, T **p)
{
    for (int i = 0; i < c->n_owned; i++) if (c->owned[i] == (void *)*p) { c->owned[i] = c->owned[--c->n_owned]; break; }
    hipFree((void *)*p); *p = NULL;
}
/* a host block released when its scope ends, on every return path (a device temporary is a DevBuf) */
template <class T> struct HostTmp {      /* NULL when there is no memory */
    T *p;
    explicit HostTmp(size_t n) : p((T *)malloc(n * sizeof(T))) {} HostTmp(const HostTmp &) = delete; ~HostTmp() { free(p); }
    operator T *() const { return p; }
};

/* glibc srand(seed) state (random_r TYPE_3): the reference draws message bits from rand() with the
 * default seed 1 (encoder.c:1838-1840) */
static void glibc_srand_state(int *st, unsigned seed)
{
    if (!seed) seed = 1;
    st[0] = (int)seed;
    for (int i = 1; i < 31; i++) {
        long hi = st[i - 1] / 127773, lo = st[i - 1] % 127773, w = 16807 * lo - 2836 * hi;
        if (w < 0) w += 2147483647;
        st[i] = (int)w;
    }
    int f = 3, b = 0;
    for (int i = 0; i < 310; i++) {
        unsigned v = (unsigned)st[f] + (unsigned)st[b];
        st[f] = (int)v;
        if (++f >= 31) f = 0;
        if (++b >= 31) b = 0;
    }
    st[31] = f; st[32] = b;
}

/* ------------------------------------------------------------------ batches */
/* Whatever a batch owns -- device memory, pinned blocks, the events of its rings, timers and window -- is a member that frees itself:
 * destroying the batch releases it all, however far its creation or a later reservation got */
extern "C" void pcamv_gpu_batch_destroy(pcamv_batch_t *b)
{
    if (!b) return;
    hipSetDevice(b->device);
    hipDeviceSynchronize();
    for (int i = 0; b->ctx && i < b->n; i++) {          /* contexts closed before the batch have taken themselves out (NULL) */
        pcamv_ctx *c = b->ctx[i];
        if (!c) continue;
        if (c->last == b) c->last = NULL;
        if (c->win == b) c->win = NULL;
        if (c->qp_owner == b) { c->qp_owner = NULL; c->qp_rows = NULL; }      /* its tables go: the context stands at the QP of its last host step */
        for (int k = 0; k < c->n_member; k++) if (c->member_of[k] == b) { c->member_of[k] = c->member_of[--c->n_member]; break; }
    }
    free(b->ctx);
    delete b;
}

/* knobs of the environment, read when a batch is made: is `name` set to `value`; an integer within [lo, hi], else dflt */
static int env_is(const char *name, const char *value) { const char *v = getenv(name); return v && !strcmp(v, value); }
static int env_int(const char *name, int lo, int hi, int dflt) { const char *v = getenv(name); return v && atoi(v) >= lo && atoi(v) <= hi ? atoi(v) : dflt; }
/* waves of a persistent dataflow kernel: as many as the device holds at once (or PCAMV_FLOW_WAVES), at least one, at most one per task */
static int flow_wave_count(int per_cu, int n_cu, size_t tasks)
{
    const char *wv = getenv("PCAMV_FLOW_WAVES");
    long waves = wv ? atol(wv) : (long)per_cu * n_cu;
    if (waves < 1) waves = 1;
    if ((size_t)waves > tasks) waves = (long)tasks;
    return (int)waves;
}
/* the n chains of a batch over the fl.nq queues, whole chains each (fl.n_mb tasks per chain) */
static void flow_split_queues(FlowDev &fl, int n)
{
    unsigned qb = 0;
    for (int q = 0; q < 8; q++) {
        const unsigned ng = q < fl.nq ? ((unsigned)n + (unsigned)(fl.nq - 1 - q)) / (unsigned)fl.nq : 0u;
        fl.qbase[q] = qb; fl.qcount[q] = ng * (unsigned)fl.n_mb; qb += fl.qcount[q];
    }
}

/* what pcamv_gpu_batch_create (below) makes of a new, empty batch; a failure leaves the clean-up to it */
static int batch_create_impl(pcamv_batch *b, pcamv_ctx_t *const *ctxs, int n)
{
    b->n = n; b->device = ctxs[0]->device; b->W = ctxs[0]->F.w; b->H = ctxs[0]->F.h;
    b->b_mbrd = ctxs[0]->F.b_mbrd;
    for (int i = 0; i < n; i++) b->b_tesa |= ctxs[i]->F.me_method == PCAMV_ME_TESA;
    b->ctx = (pcamv_ctx **)malloc(sizeof(pcamv_ctx *) * n);
    for (int i = 0; i < n; i++) b->ctx[i] = ctxs[i];
    const FrameDev &F = ctxs[0]->F;
    const int sub8x8 = (ctxs[0]->p.inter & PCAMV_ANALYSE_PSUB8x8) != 0;
    b->n_diag = F.mb_w + 2 * (F.mb_h - 1);
    b->max_diag = (F.mb_w + 1) / 2 < F.mb_h ? (F.mb_w + 1) / 2 : F.mb_h;
    b->slots_per_mb = sub8x8 ? 16 : 2;
    /* schedule: PCAMV_SCHED=diag keeps one launch per anti-diagonal (+ separate RCA / encode launches);
     * the default is the dataflow kernel.  Both are the same per-macroblock code. */
    b->sched_flow = !env_is("PCAMV_SCHED", "diag") && F.n_mb <= 65535 && n <= 65535;
    { const int ns = env_int("PCAMV_STC_STATES", 2, 4, 0); b->stc_ns = ns == 2 || ns == 4 ? ns : (n >= 1024 ? 4 : 2); }      /* trellis states per thread of the forward Viterbi */
    b->sp_lds_cols = env_int("PCAMV_SLICE_LDS_COLS", 0, SP_LDS_COLS, SP_LDS_COLS);      /* (tests: 0 sends every picture through the global scratch rows) */
    for (int k = 0; k < KT_N; k++) { b->kt[k].cap = k == KT_ANALYSE ? NEV : NKEV; b->kt[k].weight = 1; }
    if (!b->sched_flow) b->kt[KT_ANALYSE].weight = b->n_diag;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(b->h_F.room(b, (size_t)n * NRING)); TRY(b->h_E.room(b, (size_t)n * NRING));
    TRY(b->d_F.room(b, (size_t)n * NRING)); TRY(b->d_E.room(b, (size_t)n * NRING));
    if (b->sched_flow) {
        const size_t total = (size_t)n * F.n_mb;
        TRY(b->d_flow.room(b, FLOW_CTR_WORDS + 2 * total + (size_t)FLOW_RDONE_STRIDE * n));
        /* the analysis: its queues, which build of it, how many waves */
        FlowDev &fl = b->fl;
        fl.ctr = b->d_flow; fl.queue = b->d_flow + FLOW_CTR_WORDS; fl.dep = (int *)(b->d_flow + FLOW_CTR_WORDS + total);
        fl.rdone = b->d_flow + FLOW_CTR_WORDS + 2 * total; fl.spec = 0;
        fl.total = (unsigned)total; fl.spin_limit = 4u << 20;
        fl.n_gop = n; fl.n_mb = F.n_mb; fl.mb_w = F.mb_w; fl.mb_h = F.mb_h; fl.fused = 1; fl.unit = 1;
        fl.nq = env_is("PCAMV_FLOW_AFFINITY", "0") || n < 8 ? 1 : 8;
        flow_split_queues(fl, n);
        /* one chain per frame: the context states (CABAC), or -- sub-8x8 partitions priced by x264_rd_cost_part -- the non-zero counts
         * / MV differences the macroblock coded before this one leaves in the cache (PCAMV_CHAIN_NZ) */
        fl.raster = F.b_mbrd && (F.b_cabac || sub8x8);
        int per_cu = 0, n_cu = 0;
        HIPCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_analyse_flow, 64, 0));
        HIPCHK(b, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, b->device));
        if (F.b_mbrd) {
            /* which build of the RD instance (pcamv_rd_select.h: the rules and what was measured) */
            b->rd = &rd_builds[rd_select(n, n_cu, fl.raster, F.mb_w, sub8x8, b->b_tesa, getenv("PCAMV_RD_INSTANCE"), getenv("PCAMV_FLOW_SPEC"))];
            fl.spec = b->rd->spec != 0;
            per_cu = b->rd->waves_per_cu();
            if (per_cu < 0) return fail(b, PCAMV_EHIP, "the occupancy of the RD instance's build could not be read");
        }
        b->flow_waves = flow_wave_count(per_cu, n_cu, total);
        /* the second pass can take `unit` macroblocks of a row per task (PCAMV_PASS2_UNIT; the dependency graph is the
         * same on the coarser grid).  Measured at G=256: 115.1 / 114.7 / 116.9 / 122.6 ms per step for 1 / 2 / 4 / 8 --
         * its queue traffic is not what bounds it any more.  With thousands of GOPs in flight it is again: 4096 GOPs 2300 / 2277 /
         * 2264 / 2253 ms per step.  Round 3: a task's macroblocks are one LDS tile (P2Unit: one memory round trip, whole cache lines), which is
         * what the run is for now -- 1080p, ms per step for 1 / 8: 1 GOP 316 / 319, 256 GOPs 354 / 353, 512 GOPs 391 / 382, 4096 GOPs: the
         * kernel alone 106 (macroblock by macroblock) -> 65.  Default: 8 from 256 GOPs on, else 1.  Same buffers: the two kernels never overlap. */
        const int unit = env_int("PCAMV_PASS2_UNIT", 1, 8, n >= 256 ? 8 : 1);
        FlowDev &fl2 = b->fl2;      /* the analysis' queues on the coarser grid */
        fl2 = fl; fl2.unit = unit; fl2.raster = 0; fl2.spec = 0; fl2.mb_w = (F.mb_w + unit - 1) / unit; fl2.n_mb = fl2.mb_w * F.mb_h;
        fl2.total = (unsigned)n * (unsigned)fl2.n_mb;
        flow_split_queues(fl2, n);
        fl2.dep = (int *)(b->d_flow + FLOW_CTR_WORDS + fl2.total);
        HIPCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pass2_deblock_flow, 64, 0));
        b->flow2_waves = flow_wave_count(per_cu, n_cu, fl2.total);
        HIPCHK(b, hipMemset(b->d_flow, 0, FLOW_CTR_WORDS * sizeof(unsigned)));
    }
    /* the contexts learn of the batch (one that is refused below takes itself out of their lists again: pcamv_gpu_batch_destroy) */
    for (int i = 0; i < n; i++) if (ctxs[i]->n_member >= 16) return PCAMV_EINVAL;
    for (int i = 0; i < n; i++) ctxs[i]->member_of[ctxs[i]->n_member++] = b;
    for (int i = 0; i < n; i++)         /* the kernel instance with --me tesa compiled in exists for the dataflow schedule only */
        if ((ctxs[i]->F.me_method == PCAMV_ME_TESA || ctxs[i]->F.b_mbrd) && !b->sched_flow) return PCAMV_EUNSUP;     /* ... and so does the RD mode decision */
    return 0;
}
extern "C" int pcamv_gpu_batch_create(pcamv_ctx_t *const *ctxs, int n, pcamv_batch_t **out)
{
    if (!ctxs || n <= 0 || !out) return PCAMV_EINVAL;
    *out = NULL;
    for (int i = 0; i < n; i++)
        if (!ctxs[i] || ctxs[i]->device != ctxs[0]->device || ctxs[i]->F.w != ctxs[0]->F.w || ctxs[i]->F.h != ctxs[0]->F.h ||
            ctxs[i]->p.inter != ctxs[0]->p.inter || ctxs[i]->F.b_mbrd != ctxs[0]->F.b_mbrd || ctxs[i]->F.b_cabac != ctxs[0]->F.b_cabac) return PCAMV_EINVAL;
    pcamv_batch *b = new (std::nothrow) pcamv_batch();      /* (value-initialised: every field zero, every buffer empty) */
    if (!b) return PCAMV_ENOMEM;
    const int rc = batch_create_impl(b, ctxs, n);
    if (rc) { pcamv_gpu_batch_destroy(b); return rc; }      /* one cleanup path: whatever was allocated so far is released */
    *out = b;
    return 0;
}
extern "C" const char *pcamv_gpu_batch_last_error(const pcamv_batch_t *b) { return b ? b->err : "no batch"; }
extern "C" int pcamv_gpu_batch_set_closed_loop(pcamv_batch_t *b, int on) { if (!b) return PCAMV_EINVAL; b->closed_loop = on != 0; return 0; }
static int flow_check(pcamv_batch *b);
extern "C" int pcamv_gpu_fetch_recon(pcamv_ctx_t *c, uint8_t *const planes[3])
{
    if (!c || !planes) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    TRY(on_behalf(c, c->last, flow_check(c->last)));
    const size_t ysz = (size_t)c->F.w * c->F.h;
    for (int i = 0; i < 3; i++)
        if (planes[i]) HIPCHK(c, hipMemcpy(planes[i], c->F.rec[i], i ? ysz / 4 : ysz, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int pcamv_gpu_recon_device(pcamv_ctx_t *c, void *planes[3])
{
    if (!c || !planes) return PCAMV_EINVAL;
    for (int i = 0; i < 3; i++) planes[i] = c->F.rec[i];
    return 0;
}
static const char *dominant_kernel(const pcamv_batch *b)
{
    if (!b || !b->sched_flow) return "k_search_diag";
    if (b->b_mbrd) return "k_analyse_flow_rd";       /* (what batch_create saw: contexts may have been closed since, their slots are NULL) */
    if (b->b_tesa) return "k_analyse_flow_tesa";
    return "k_analyse_flow";
}
extern "C" const char *pcamv_gpu_batch_dominant_kernel(const pcamv_batch_t *b) { return dominant_kernel(b); }
static const char *kt_name(const pcamv_batch *b, int k)      /* what pcamv_gpu_batch_kernel_time knows timer k by */
{
#define KT_NAME(id, name) name,
    static const char *const small[KT_N] = {PCAMV_TIMERS(KT_NAME)};
#undef KT_NAME
    return k == KT_ANALYSE ? dominant_kernel(b) : small[k];
}
extern "C" int pcamv_gpu_batch_copy_results_async(pcamv_batch_t *b, void *dst_mb, size_t mb_stride, void *dst_flip, size_t flip_stride, void *stream)
{
    if (!b || !dst_mb) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(batch_live(b));
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        const size_t nb = (size_t)c->F.n_mb * sizeof(pcamv_mb_t);
        if (mb_stride < nb || (dst_flip && flip_stride < (size_t)c->cap)) return PCAMV_EINVAL;
        HIPCHK(b, hipMemcpyAsync((char *)dst_mb + (size_t)i * mb_stride, c->F.rec_mb, nb, hipMemcpyDefault, st));
        if (dst_flip) HIPCHK(b, hipMemcpyAsync((char *)dst_flip + (size_t)i * flip_stride, c->d_flip, (size_t)c->cap, hipMemcpyDefault, st));
    }
    return 0;
}

/* ------------------------------------------------------------------ contexts */
extern "C" void pcamv_gpu_close(pcamv_ctx_t *c);

static int open_impl(pcamv_ctx *c, const pcamv_params_t *p, int device);
extern "C" int pcamv_gpu_open(const pcamv_params_t *p, int device, pcamv_ctx_t **out)
{
    if (!p || !out) return PCAMV_EINVAL;
    *out = NULL;
    if (p->i_width <= 0 || p->i_height <= 0 || p->i_width % 16 || p->i_height % 16) return PCAMV_EINVAL;
    if (p->i_subpel_refine < 1 || p->i_subpel_refine > 7) return PCAMV_EUNSUP;   /* 8, 9: RD refinement of the MVs (disabled in the fork's P frames anyway, analyse.c:3112) */
    if (p->i_me_method < PCAMV_ME_DIA || p->i_me_method > PCAMV_ME_TESA) return PCAMV_EUNSUP;
    if (p->i_me_method == PCAMV_ME_TESA && p->i_me_range > TESA_MAX_RANGE) return PCAMV_EUNSUP;      /* the survivor list lives in LDS: 32 x 33 positions */
    /* x264_validate_parameters leaves 32 .. 512 here (encoder.c:561), but the analysis is defined for smaller ranges as well (the clip bounds of
     * analyse.c:271-317 only move inwards) and the parity tests drive it at 16, where the bounds are easiest to reach: refused below that */
    if (p->i_me_range < 4 || p->i_me_range > 64 || p->i_mv_range < 16) return PCAMV_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PCAMV_ENODEV;
    pcamv_ctx *c = new (std::nothrow) pcamv_ctx();
    if (!c) return PCAMV_ENOMEM;
    memset((void *)c, 0, sizeof(*c));
    c->p = *p; c->device = device; c->last_field = 1;
    const int rc = open_impl(c, p, device);
    if (rc) { pcamv_gpu_close(c); return rc; }          /* one cleanup path: whatever was allocated so far is released */
    *out = c;
    return 0;
}
static int open_impl(pcamv_ctx *c, const pcamv_params_t *p, int device)
{
    HIPCHK(c, hipSetDevice(device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    FrameDev &F = c->F;
    pcamv_frame_set_params(&F, p);
    const size_t ysz = (size_t)F.w * F.h, lsz = (size_t)F.plane_size, csz = (size_t)F.cstride * F.clines, n_mb = (size_t)F.n_mb;
    EmbedDev &E = c->E;
    for (int i = 0; i < 3; i++) {
        TRY(ctx_alloc(c, &c->d_fenc[i], (i ? ysz / 4 : ysz) + PCAMV_SRC_GUARD));     /* (guard bytes behind the plane: pcamv_gpu_debug_fetch_fenc) */
        HIPCHK(c, hipMemset(c->d_fenc[i] + (i ? ysz / 4 : ysz), SRC_GUARD_BYTE, PCAMV_SRC_GUARD));
        TRY(ctx_alloc(c, &c->d_raw[i], i ? ysz / 4 : ysz));
        TRY(ctx_alloc(c, &F.rec[i], i ? ysz / 4 : ysz));
        F.fenc[i] = c->d_fenc[i]; F.raw[i] = c->d_raw[i];
    }
    TRY(ctx_alloc(c, &F.luma_base, 4 * lsz + 64, 0));      /* the repeated columns of each plane's last strip are never written */
    if (F.me_method == PCAMV_ME_ESA || F.me_method == PCAMV_ME_TESA) TRY(ctx_alloc(c, &F.luma_raster, (size_t)F.stride * F.lines + 64));
    TRY(ctx_alloc(c, &F.chroma_base[0], 2 * (csz + 64))); F.chroma_base[1] = F.chroma_base[0] + csz + 64;   /* one allocation: 32-bit offsets reach both */
    F.cplane_size = (long long)(csz + 64);
    for (int k = 0; k < 2; k++) F.chroma[k] = F.chroma_base[k] + (size_t)F.cstride * PCAMV_CPAD + PCAMV_CPAD;
    TRY(ctx_alloc(c, &F.mb_type, n_mb)); TRY(ctx_alloc(c, &c->d_ref8, n_mb * 4)); TRY(ctx_alloc(c, &c->d_prev_ref, n_mb * 4));
    TRY(ctx_alloc(c, &c->d_mv, n_mb * 32, 0)); TRY(ctx_alloc(c, &c->d_prev_mv, n_mb * 32));
    TRY(ctx_alloc(c, &c->d_mv_b, n_mb * 32, 0)); TRY(ctx_alloc(c, &c->d_ref8_b, n_mb * 4, 0xff));
    TRY(ctx_alloc(c, &F.mvr, n_mb * 2, 0)); TRY(ctx_alloc(c, &F.mvp_aux, n_mb * 32, 0));
    TRY(ctx_alloc(c, &F.rec_mb, n_mb, 0));
    F.mv = c->d_mv; F.ref8 = c->d_ref8; F.prev_mv = c->d_prev_mv; F.prev_ref = c->d_prev_ref; F.have_prev = 0;
    c->cap = 16 * F.n_mb;
    const size_t cap = (size_t)c->cap;
    TRY(ctx_alloc(c, &E.cover, cap)); TRY(ctx_alloc(c, &E.stego, cap)); TRY(ctx_alloc(c, &E.message, cap));
    TRY(ctx_alloc(c, &c->d_user_msg, cap)); TRY(ctx_alloc(c, &E.colinfo, cap));
    TRY(ctx_alloc(c, &E.rho, cap)); TRY(ctx_alloc(c, &c->d_flip, cap));
    TRY(ctx_alloc(c, &E.hdr, 8, 0)); TRY(ctx_alloc(c, &E.rnd, 40)); TRY(ctx_alloc(c, &E.cols, 2 * STC_MAXW + 8)); TRY(ctx_alloc(c, &E.lcg, 1));
    TRY(ctx_alloc(c, &E.path, cap * 32));
    TRY(ctx_alloc(c, &F.nnz, n_mb, 0)); TRY(ctx_alloc(c, &E.car_base, n_mb, 0)); TRY(ctx_alloc(c, &c->d_flip_user, cap));
    TRY(ctx_alloc(c, &c->d_mbflip, n_mb, 1));
    if (F.b_mbrd) {
        uint32_t *d_tab;
        TRY(ctx_alloc(c, &F.nb_nz, n_mb * 16, 0)); TRY(ctx_alloc(c, &F.nb_cbp, n_mb, 0)); TRY(ctx_alloc(c, &F.nb_mvd, n_mb * 16, 0));
        TRY(ctx_alloc(c, &F.cabac, PCAMV_CHAIN_BYTES, 0)); TRY(ctx_alloc(c, &d_tab, 256));
        uint32_t tab[256]; pcamv_build_cabac_tab(tab);
        HIPCHK(c, hipMemcpy(d_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
        F.cabac_tab = d_tab;
    }
    int rnd[40]; memset(rnd, 0, sizeof(rnd)); glibc_srand_state(rnd, 1);
    HIPCHK(c, hipMemcpy(E.rnd, rnd, sizeof(rnd), hipMemcpyHostToDevice));
    long long lcg = 1; HIPCHK(c, hipMemcpy(E.lcg, &lcg, sizeof(lcg), hipMemcpyHostToDevice));
    const long long pstate[PST_WORDS] = {0, 0, 0, 1};       /* cursors at 0; the receiver's column generator starts like the sender's */
    TRY(ctx_alloc(c, &E.pstate, PST_WORDS)); HIPCHK(c, hipMemcpy(E.pstate, pstate, sizeof(pstate), hipMemcpyHostToDevice));
    F.car_base = E.car_base; F.flip = c->d_flip; F.mbflip = c->d_mbflip;
    E.mbs = F.rec_mb; E.n_mb = F.n_mb; E.mbflip = c->d_mbflip; E.flip = c->d_flip; E.cap = c->cap;
    E.user_message = NULL; E.user_message_len = 0; E.emrate = 0; E.payload = NULL; E.payload_bits = 0;
    c->X.n_mb = F.n_mb; c->X.cap = c->cap; c->X.pstate = E.pstate;
    pcamv_ctx *one[1] = {c};
    return pcamv_gpu_batch_create(one, 1, &c->self);
}

extern "C" void pcamv_gpu_close(pcamv_ctx_t *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->self) pcamv_gpu_batch_destroy(c->self);
    for (int k = 0; k < c->n_member; k++) {             /* batches that outlive this context must not touch it again */
        pcamv_batch *b = c->member_of[k];
        for (int i = 0; i < b->n; i++) if (b->ctx[i] == c) b->ctx[i] = NULL;
    }
    for (int i = 0; i < c->n_owned; i++) hipFree(c->owned[i]);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

/* the per-QP tables of a context (MV bit costs; --subme >= 6: the context states at the slice start), made on first use and kept */
static int ensure_qp_tables(pcamv_ctx *c, int qp)
{
    if (qp < 0 || qp > 51) return fail(c, PCAMV_EINVAL, "qp %d out of range", qp);
    if (!c->d_cost_mv[qp]) {
        HostTmp<int16_t> h(PCAMV_COST_MV_LEN);
        if (!h) return fail(c, PCAMV_ENOMEM, "cost table");
        pcamv_build_cost_mv(qp, h);
        TRY(ctx_alloc(c, &c->d_cost_mv[qp], (size_t)PCAMV_COST_MV_LEN + 1));      /* + 1: prim_mv_cost fetches the dword that holds an entry */
        HIPCHK(c, hipMemcpy(c->d_cost_mv[qp], h, PCAMV_COST_MV_LEN * sizeof(int16_t), hipMemcpyHostToDevice));
    }
    if (c->F.b_mbrd && !c->d_cabac_init[qp]) {       /* context states at the slice start for this QP (x264_cabac_context_init, encoder.c:1227) */
        uint8_t init[PCAMV_CHAIN_BYTES] = {0};       /* states, then nothing left over from an earlier macroblock */
        pcamv_build_cabac_init(qp, init);
        TRY(ctx_alloc(c, &c->d_cabac_init[qp], (size_t)PCAMV_CHAIN_BYTES));
        HIPCHK(c, hipMemcpy(c->d_cabac_init[qp], init, PCAMV_CHAIN_BYTES, hipMemcpyHostToDevice));
    }
    return 0;
}
/* the QP-dependent part of a frame descriptor of context c, from the context's tables for that QP: of the context's own descriptor for
 * an analysis or a step (ensure_qp), of a probe's private copy for a probe (probe_frame) */
static void frame_use_qp(const pcamv_ctx *c, FrameDev *F, int qp)
{
    pcamv_frame_set_qp(F, &c->p, qp);
    F->cost_mv = c->d_cost_mv[qp] + PCAMV_COST_MV_CENTRE;
    if (F->b_mbrd) F->cabac_init = c->d_cabac_init[qp];
}
/* an analysis or a step at this QP: it becomes the context's, the one pass 2, the loop filter and the writers work at until the next */
static int ensure_qp(pcamv_ctx *c, int qp)
{
    TRY(ensure_qp_tables(c, qp));
    frame_use_qp(c, &c->F, qp);
    c->qp_rows = NULL; c->qp_owner = NULL;      /* a QP in force on the device ends here */
    return 0;
}
/* The frame descriptor of a probe (block_costs, rd_probe): a copy of the context's with the probe's QP, on the device for the probe's
 * one launch.  The context keeps its own QP, so whatever runs on it after the probe computes what it would have without it. */
static int probe_frame(pcamv_ctx *c, int qp, DevBuf<FrameDev> &d_F)
{
    TRY(ensure_qp_tables(c, qp));
    TRY(d_F.room(c, 1));
    FrameDev hF = c->F; hF.self = d_F;
    frame_use_qp(c, &hF, qp);
    HIPCHK(c, hipMemcpy(d_F, &hF, sizeof(FrameDev), hipMemcpyHostToDevice));
    return 0;
}
/* The second pass may take the first pass' pixels and non-zero flags for a macroblock whose motion did not change (mbk_pass2) only while
 * records, source, reference planes and quantiser are what the first pass saw: whatever replaces one of them between an analysis and
 * pcamv_gpu_pass2_pframe calls this, and so does a step found incomplete. */
static void drop_rec_reuse(pcamv_ctx *c) { c->rec_pristine = 0; }
/* diagnostics (parity tests): FNV-1a of the 460 CABAC context states after every macroblock of the following analyses */
extern "C" int pcamv_gpu_debug_state_hash(pcamv_ctx_t *c, int enable)
{
    if (!c) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (enable && !c->d_dbg_hash) TRY(ctx_alloc(c, &c->d_dbg_hash, (size_t)c->F.n_mb, 0));
    c->F.dbg_hash = enable ? c->d_dbg_hash : NULL;
    return 0;
}
extern "C" int pcamv_gpu_debug_state_hash_fetch(pcamv_ctx_t *c, uint32_t *out)
{
    if (!c || !out || !c->d_dbg_hash) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, c->d_dbg_hash, (size_t)c->F.n_mb * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pcamv_gpu_upload_fenc(pcamv_ctx_t *c, const uint8_t *const plane[3], const int stride[3])
{
    if (!c || !plane || !stride) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < 3; i++) {
        int w = c->F.w >> !!i, h = c->F.h >> !!i;
        HIPCHK(c, hipMemcpy2D(c->d_fenc[i], w, plane[i], stride[i], w, h, hipMemcpyHostToDevice));   /* caller memory is pageable: blocking copy */
        c->F.fenc[i] = c->d_fenc[i];
    }
    drop_rec_reuse(c);          /* a new source: a second pass re-encodes every macroblock on it */
    return 0;
}
extern "C" int pcamv_gpu_set_fenc_device(pcamv_ctx_t *c, const void *y, const void *u, const void *v)
{
    if (!c || !y || !u || !v) return PCAMV_EINVAL;
    c->F.fenc[0] = (const uint8_t *)y; c->F.fenc[1] = (const uint8_t *)u; c->F.fenc[2] = (const uint8_t *)v;
    drop_rec_reuse(c);
    return 0;
}

/* ------------------------------------------------------------------ batched launches */
/* the ring's next slot, once its descriptors are no longer in flight */
template <int N> static int ring_take(pcamv_batch *b, EvRing<N> &r, int *slot_out)
{
    const int slot = r.head;
    r.head = (slot + 1) % N;
    if (!r.done[slot]) HIPCHK(b, hipEventCreateWithFlags(&r.done[slot], hipEventDisableTiming));
    if (r.used[slot]) HIPCHK(b, hipEventSynchronize(r.done[slot]));
    *slot_out = slot;
    return 0;
}
/* ... and what was queued on `st` so far is what reads them */
template <int N> static int ring_release(pcamv_batch *b, EvRing<N> &r, int slot, hipStream_t st)
{
    HIPCHK(b, hipEventRecord(r.done[slot], st));
    r.used[slot] = 1;
    return 0;
}
/* the staging ring's buffer k with room for `total` bytes and `spare` more where it has to grow; host == 0: the device side alone.
 * The only place that sizes a ring's buffers.  Growing frees, which waits for the device: an index call sizes su_stage behind its
 * synchronisation; the rings of host slices and headers grow inside the call that outgrows them (stage_take) */
static int stage_room(pcamv_batch *b, StageRing &R, int k, size_t total, size_t spare, int host)
{
    if (total <= R.d[k].cap && (!host || total <= R.h[k].cap)) return 0;       /* (both sides: a side that could not be made is empty, and is made again here) */
    if (host) TRY(R.h[k].room(b, total + spare));
    return R.d[k].room(b, total + spare);
}
/* the staging ring's next buffer with room for `total` bytes (regrown with a quarter to spare), once it is no longer in flight */
static int stage_take(pcamv_batch *b, StageRing &R, size_t total, int *k_out, int host = 1)
{
    TRY(ring_take(b, R.ring, k_out));
    return stage_room(b, R, *k_out, total, total / 4, host);
}
/* what was queued on `st` so far is what reads buffer k: called once the kernels that read its device side are queued */
static int stage_release(pcamv_batch *b, StageRing &R, int k, hipStream_t st) { return ring_release(b, R.ring, k, st); }
/* the first `total` bytes of buffer k to the device, one copy on `st`.  From here on the buffer is in flight whatever happens to the
 * kernels: the event stands for the copy until stage_release moves it behind the kernels that read the device side */
static int stage_send(pcamv_batch *b, StageRing &R, int k, size_t total, hipStream_t st)
{
    HIPCHK(b, hipMemcpyAsync(R.d[k], R.h[k], total, hipMemcpyHostToDevice, st));
    return stage_release(b, R, k, st);
}
/* the job arrays in front of a stream step's RBSP slots: [off n][len n][start_bit n] int64, [qp n][first n][frame_num n][nal_header n][entropy n] int32
 * (entropy: what k_slice_header_sets alone writes, the mode of the entry each header was read under) */
static size_t stream_step_hdr(int n) { return ((size_t)n * (3 * 8 + 5 * 4) + 15) & ~(size_t)15; }
static void batch_push_qp(pcamv_batch *b, hipStream_t st, int slot);
/* take the next descriptor slot, fill it from the contexts' current FrameDev/EmbedDev and queue its upload; where a context has a QP
 * in force on the device, the patch behind it (batch_push_qp) */
static int batch_push_descs(pcamv_batch *b, hipStream_t st, const FrameDev **dF, const EmbedDev **dE, int *slot_out)
{
    int slot, patch = 0;
    for (int i = 0; i < b->n && !patch; i++) patch = b->ctx[i]->qp_rows != NULL;
    if (patch && !b->h_Q) TRY(b->h_Q.room(b, (size_t)b->n * NRING));          /* (before a slot is taken: a slot taken is a slot released by the caller) */
    if (patch && !b->d_Q) TRY(b->d_Q.room(b, (size_t)b->n * NRING));
    TRY(ring_take(b, b->ring, &slot));
    FrameDev *hF = b->h_F + (size_t)slot * b->n; EmbedDev *hE = b->h_E + (size_t)slot * b->n;
    for (int i = 0; i < b->n; i++) { hF[i] = b->ctx[i]->F; hF[i].self = b->d_F + (size_t)slot * b->n + i; hE[i] = b->ctx[i]->E; }
    if (b->d_msg) for (int i = 0; i < b->n; i++) { hE[i].payload = b->d_msg; hE[i].payload_bits = b->msg_bits; }       /* one message for the batch: k_message_plan sets every cursor */
    HIPCHK(b, hipMemcpyAsync(b->d_F + (size_t)slot * b->n, hF, sizeof(FrameDev) * b->n, hipMemcpyHostToDevice, st));
    HIPCHK(b, hipMemcpyAsync(b->d_E + (size_t)slot * b->n, hE, sizeof(EmbedDev) * b->n, hipMemcpyHostToDevice, st));
    *dF = b->d_F + (size_t)slot * b->n; *dE = b->d_E + (size_t)slot * b->n; *slot_out = slot;
    if (patch) batch_push_qp(b, st, slot);       /* (an upload that fails shows in the caller's launched(): the slot is handed out either way) */
    return 0;
}

/* one launch per anti-diagonal d = x + 2 y of the macroblock grid (left / top / top-right dependency): launch(macroblocks on it, d) */
template <class Launch> static void diag_launch(int n_diag, const FrameDev &F, Launch launch)
{
    for (int d = 0; d < n_diag; d++) {
        int y_lo = d - (F.mb_w - 1); y_lo = y_lo > 0 ? (y_lo + 1) >> 1 : 0;
        int y_hi = d / 2; if (y_hi > F.mb_h - 1) y_hi = F.mb_h - 1;
        int cnt = y_hi - y_lo + 1;
        if (cnt <= 0) continue;
        launch(cnt, d);
    }
}

/* A timed launch: the events of timer k around what `launch` queues on `st`, the only place that records them.  A timer whose events
 * cannot be made stays off, and its launches go untimed */
template <class Launch> static void timed(pcamv_batch *b, int k, hipStream_t st, Launch launch)
{
    KTimer &T = b->kt[k];
    if (!T.made) {
        T.made = 1;
        for (int i = 0; i < T.cap && T.made > 0; i++) if (hipEventCreate(&T.e0[i]) != hipSuccess || hipEventCreate(&T.e1[i]) != hipSuccess) T.made = -1;
    }
    if (T.made < 0) { launch(); return; }
    hipEventRecord(T.e0[T.head], st);
    launch();
    hipEventRecord(T.e1[T.head], st);
    T.head = (T.head + 1) % T.cap; if (T.n < T.cap) T.n++;
}
/* ... of one kernel of this unit */
template <class Kernel, class... Args> static void timed_kernel(pcamv_batch *b, int k, hipStream_t st, Kernel kernel, dim3 grid, dim3 block, const Args &... args)
{
    timed(b, k, st, [&] { hipLaunchKernelGGL(kernel, grid, block, 0, st, args...); });
}

/* The patch behind the upload of descriptor slot `slot`: the jobs of the batch's contexts in the slot of their own ring (made once for
 * good by the first push that needs it, batch_push_descs), then k_frame_qp.  A context without a QP in force has an empty job */
static void batch_push_qp(pcamv_batch *b, hipStream_t st, int slot)
{
    QpJob *hQ = b->h_Q + (size_t)slot * b->n, *dQ = b->d_Q + (size_t)slot * b->n;
    for (int i = 0; i < b->n; i++) {
        const pcamv_ctx *c = b->ctx[i];
        hQ[i].cell = c->qp_rows ? c->d_qp_cell : NULL; hQ[i].rows = c->qp_rows; hQ[i].src = c->qp_rows && b->qp_src ? b->qp_src + i : NULL;
    }
    hipMemcpyAsync(dQ, hQ, sizeof(QpJob) * b->n, hipMemcpyHostToDevice, st);
    timed_kernel(b, KT_FRAME_QP, st, k_frame_qp, dim3((unsigned)b->n), dim3(64), b->d_F + (size_t)slot * b->n, (const QpJob *)dQ);
}

/* the second pass takes the frame's reconstruction as it stands: the first pass' own, once (then it has been filtered in place) */
static void pass2_takes_rec(pcamv_ctx *c)
{
    c->F.rec_is_pass1 = c->rec_pristine;
    c->rec_pristine = 0;
}

/* the stages `what` (ST_*) of one step of every context of the batch, queued on `st` */
static int batch_launch(pcamv_batch *b, int what, hipStream_t st)
{
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        if ((what & ST_ANALYSE) && c->prev_internal) {      /* this frame writes the field the last analysis did not write, and reads that one */
            const int wr = !c->last_field;
            c->F.mv = wr ? c->d_mv_b : c->d_mv; c->F.ref8 = wr ? c->d_ref8_b : c->d_ref8;
            c->F.prev_mv = wr ? c->d_mv : c->d_mv_b; c->F.prev_ref = wr ? c->d_ref8 : c->d_ref8_b;
        }
        if (what & ST_ANALYSE) c->last_field = c->F.mv == c->d_mv_b;
        if (what & ST_ANALYSE) c->rec_pristine = 1;         /* the analysis leaves the first pass' reconstruction + non-zero flags in rec / nnz ... */
        if (what & ST_PASS2) pass2_takes_rec(c);            /* ... until a second pass has filtered the picture in place */
        else c->F.rec_is_pass1 = 0;
    }
    const FrameDev *dF; const EmbedDev *dE; int slot;
    TRY(batch_push_descs(b, st, &dF, &dE, &slot));
    const FrameDev &F = b->ctx[0]->F;
    const unsigned G = (unsigned)b->n;
    if (what & ST_PLANES) {
        /* a wave = 8 strips (those that begin inside the stride) x HP_ROWS lines; lines is a multiple of 16 */
        dim3 g(((F.stride + PCAMV_LSW - 1) / PCAMV_LSW + 7) / 8, (F.lines + HP_ROWS - 1) / HP_ROWS, G);
        hipLaunchKernelGGL(k_hpel, g, dim3(HP_THREADS), 0, st, dF);
        dim3 gc((F.cstride / 16 * CP_ROWS + CP_THREADS - 1) / CP_THREADS, (F.clines + CP_ROWS - 1) / CP_ROWS, 2 * G);
        hipLaunchKernelGGL(k_chroma_pad, gc, dim3(CP_THREADS), 0, st, dF);
    }
    if (what & ST_ANALYSE) {
        for (int i = 0; i < b->n; i++) b->ctx[i]->last = b;
        if (b->sched_flow) {        /* timed: the analysis kernel without k_flow_init */
            hipLaunchKernelGGL(k_flow_init, dim3((b->fl.total + 255) / 256), dim3(256), 0, st, b->fl);
            timed(b, KT_ANALYSE, st, [&] {
                if (b->b_mbrd) b->rd->launch((unsigned)b->flow_waves, st, dF, b->fl);
                else if (b->b_tesa) pcamv_launch_flow_tesa((unsigned)b->flow_waves, st, dF, b->fl);
                else hipLaunchKernelGGL(k_analyse_flow, dim3(b->flow_waves), dim3(64), 0, st, dF, b->fl);
            });
        } else {                    /* timed: the n_diag launches of the search (one pair of events, KTimer::weight), without k_rca / k_encode */
            timed(b, KT_ANALYSE, st, [&] {
                diag_launch(b->n_diag, F, [&](int cnt, int d) { hipLaunchKernelGGL(k_search_diag<0>, dim3(cnt, G), dim3(64), 0, st, dF, d); });
            });
            hipLaunchKernelGGL(k_rca, dim3(F.n_mb * b->slots_per_mb, G), dim3(64), 0, st, dF, b->slots_per_mb);
            hipLaunchKernelGGL(k_encode, dim3(F.n_mb, G), dim3(64), 0, st, dF);
        }
    }
    if ((what & ST_EMBED) && b->d_msg) {     /* every context's m, then the place of each in the message: pstate[PST_TX], which k_embed_prepare reads */
        timed_kernel(b, KT_MESSAGE_COUNT, st, k_message_count, dim3(G), dim3(256), dE, b->d_mtx_m);
        timed_kernel(b, KT_MESSAGE_PLAN, st, k_message_plan, dim3(1), dim3(MSG_PLAN_THREADS), b->d_mtx_m, (const int *)NULL, b->n, 1, PCAMV_MSG_NO_CAP, b->d_mtx, b->d_mtx_at, dE);
    }
    if (what & ST_EMBED) {
        timed_kernel(b, KT_EMBED_PREPARE, st, k_embed_prepare, dim3(G), dim3(1024), dE);
        /* 2 trellis states per thread: measured 3.25 / 2.89 / 2.90 ms per 1080p frame for 1 / 2 / 4 */
        /* (one frame alone: 2 trellis states per thread is the fastest chain; thousands of frames: 4 states per thread = 4 waves per frame, so
         * that a CU holds eight frames' trellises instead of four and the batch needs half the rounds: 18.6 -> 13.3 ms per 4096-frame step) */
        if (b->stc_ns == 4) hipLaunchKernelGGL(k_stc_forward<4>, dim3(G), dim3(256), 0, st, dE);
        else hipLaunchKernelGGL(k_stc_forward<2>, dim3(G), dim3(512), 0, st, dE);
        hipLaunchKernelGGL(k_stc_backward, dim3(G), dim3(64), 0, st, dE);
        hipLaunchKernelGGL(k_mb_flips, dim3((F.n_mb + 255) / 256, G), dim3(256), 0, st, dE);
    }
    if (what & ST_PASS2) {      /* final MVs -> reconstruction -> loop filter, same dependency as the search */
        if (b->sched_flow) {
            hipLaunchKernelGGL(k_flow_init, dim3((b->fl2.total + 255) / 256), dim3(256), 0, st, b->fl2);
            hipLaunchKernelGGL(k_pass2_deblock_flow, dim3(b->flow2_waves), dim3(64), 0, st, dF, b->fl2);
        } else {
            diag_launch(b->n_diag, F, [&](int cnt, int d) { pcamv_launch_pass2_diag(P2D_PASS2 | P2D_DEBLOCK, cnt, G, st, dF, d); });
        }
    }
    TRY(launched(b));
    return ring_release(b, b->ring, slot, st);
}
/* after a synchronisation: did the dataflow kernel of the last step give up on a bounded spin? */
static int flow_check(pcamv_batch *b)
{
    if (!b || !b->sched_flow) return 0;
    unsigned bad = 0;
    HIPCHK(b, hipMemcpy(&bad, b->fl.ctr + FLOW_ERR, sizeof(bad), hipMemcpyDeviceToHost));
    if (bad) {
        hipMemset(b->fl.ctr + FLOW_ERR, 0, sizeof(unsigned));
        for (int i = 0; i < b->n; i++) if (b->ctx[i]) drop_rec_reuse(b->ctx[i]);      /* no first pass' reconstruction to speak of */
        return fail(b, PCAMV_EHIP, "dataflow kernel: queue wait timed out (results of the last step are incomplete)");
    }
    return 0;
}
static int ctx_launch(pcamv_ctx *c, int what) { return on_behalf(c, c->self, batch_launch(c->self, what, c->stream)); }

extern "C" int pcamv_gpu_set_ref(pcamv_ctx_t *c, const uint8_t *const plane[3], const int stride[3], const int16_t *prev_mv, const int8_t *prev_ref)
{
    if (!c || !plane || !stride) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < 3; i++) {
        int w = c->F.w >> !!i, h = c->F.h >> !!i;
        HIPCHK(c, hipMemcpy2D(c->d_raw[i], w, plane[i], stride[i], w, h, hipMemcpyHostToDevice));
        c->F.raw[i] = c->d_raw[i];
    }
    c->F.have_prev = prev_mv != NULL && prev_ref != NULL && c->p.i_tscale != 0;
    c->F.ref_is_inter = prev_mv != NULL && prev_ref != NULL;      /* the reference picture is a P picture: its macroblock types (analyse.c:369) */
    c->prev_internal = 0;
    c->F.mv = c->d_mv; c->F.ref8 = c->d_ref8;
    c->F.prev_mv = c->d_prev_mv; c->F.prev_ref = c->d_prev_ref;
    if (c->F.have_prev) {
        HIPCHK(c, hipMemcpy(c->d_prev_mv, prev_mv, (size_t)c->F.n_mb * 64, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_prev_ref, prev_ref, (size_t)c->F.n_mb * 4, hipMemcpyHostToDevice));
    }
    drop_rec_reuse(c);          /* the planes below are the new reference's at once: a second pass re-encodes every macroblock against them */
    TRY(ctx_launch(c, ST_PLANES));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
/* (The planes the analysis and the second pass read -- luma_base, chroma_base -- are made from these by the next step's plane production;
 * F.raw is read by k_hpel / k_chroma_pad alone.  Until that step a second pass runs against the planes of the reference before, and what
 * the first pass left of it stays valid.) */
extern "C" int pcamv_gpu_set_ref_device(pcamv_ctx_t *c, const void *y, const void *u, const void *v, const void *prev_mv, const void *prev_ref)
{
    if (!c || !y || !u || !v) return PCAMV_EINVAL;
    c->F.have_prev = prev_mv != NULL && prev_ref != NULL && c->p.i_tscale != 0;
    c->F.ref_is_inter = prev_mv != NULL && prev_ref != NULL;
    c->prev_internal = prev_mv == PCAMV_PREV_FIELD_INTERNAL;
    if (c->F.have_prev && !c->prev_internal) { c->F.prev_mv = (const int16_t *)prev_mv; c->F.prev_ref = (const int8_t *)prev_ref; c->F.mv = c->d_mv; c->F.ref8 = c->d_ref8; }
    /* the filter itself runs as the first kernels of the next step (plane production is part of the
     * timed path) and reads the caller's planes in place */
    c->F.raw[0] = (const uint8_t *)y; c->F.raw[1] = (const uint8_t *)u; c->F.raw[2] = (const uint8_t *)v;
    return 0;
}

extern "C" int pcamv_gpu_get_ref_planes(pcamv_ctx_t *c, uint8_t *out, int *stride, int *lines)
{
    if (!c || !out) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    /* the device keeps the planes in strips (pcamv_common.h); the caller gets x264's raster planes */
    const size_t psz = (size_t)c->F.plane_size;
    HostTmp<uint8_t> tmp(4 * psz);
    if (!tmp) return fail(c, PCAMV_EHIP, "out of host memory");
    HIPCHK(c, hipMemcpy(tmp, c->F.luma_base, 4 * psz, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++)
        for (int y = 0; y < c->F.lines; y++)
            for (int x = 0; x < c->F.stride; x++)
                out[((size_t)k * c->F.lines + y) * c->F.stride + x] = tmp[k * psz + (size_t)y * PCAMV_LROW + x + (size_t)(x / PCAMV_LSW) * c->F.lskip];
    if (stride) *stride = c->F.stride;
    if (lines) *lines = c->F.lines;
    return 0;
}

/* diagnostics (layout tests): the four luma planes as they lie in device memory, strips and repeated columns included, then the
 * two padded chroma planes */
extern "C" int pcamv_gpu_get_ref_strips(pcamv_ctx_t *c, uint8_t *out, size_t cap, size_t *luma_bytes, size_t *chroma_bytes)
{
    if (!c) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const size_t lb = 4 * (size_t)c->F.plane_size, csz = (size_t)c->F.cstride * c->F.clines;
    if (luma_bytes) *luma_bytes = lb;
    if (chroma_bytes) *chroma_bytes = 2 * csz;
    if (!out) return 0;                                     /* sizes only */
    if (cap < lb + 2 * csz) return fail(c, PCAMV_EINVAL, "get_ref_strips: %zu bytes offered, %zu needed", cap, lb + 2 * csz);
    HIPCHK(c, hipMemcpy(out, c->F.luma_base, lb, hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; k++) HIPCHK(c, hipMemcpy(out + lb + k * csz, c->F.chroma_base[k], csz, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pcamv_gpu_analyse_pframe(pcamv_ctx_t *c, int qp, int embed, pcamv_mb_t *out_mb, uint8_t *const recon[3])
{
    if (!c || !out_mb) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_qp(c, qp));
    c->F.embed = embed;
    TRY(ctx_launch(c, ST_ANALYSE));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    TRY(on_behalf(c, c->self, flow_check(c->self)));
    HIPCHK(c, hipMemcpy(out_mb, c->F.rec_mb, (size_t)c->F.n_mb * sizeof(pcamv_mb_t), hipMemcpyDeviceToHost));
    if (recon)
        for (int i = 0; i < 3; i++)
            if (recon[i]) HIPCHK(c, hipMemcpy(recon[i], c->F.rec[i], ((size_t)c->F.w * c->F.h) >> (i ? 2 : 0), hipMemcpyDeviceToHost));
    return 0;
}

static int fetch_embed(pcamv_ctx *c, pcamv_embed_t *out)
{
    int hdr[8];
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(hdr, c->E.hdr, sizeof(hdr), hipMemcpyDeviceToHost));
    out->n = hdr[0]; out->m = hdr[1]; out->stc_ok = hdr[2]; out->num_flip = hdr[3];
    if (out->n < 0 || out->m < 0 || out->n > c->cap) return fail(c, PCAMV_EHIP, "embed header corrupt");
    const int m_copy = out->m < c->cap ? out->m : c->cap;          /* a bits-per-frame rate above the capacity: stc_embed failed (m > n), the message array holds cap bits */
    if (out->cover && out->n) HIPCHK(c, hipMemcpy(out->cover, c->E.cover, out->n, hipMemcpyDeviceToHost));
    if (out->rho && out->n) HIPCHK(c, hipMemcpy(out->rho, c->E.rho, (size_t)out->n * 4, hipMemcpyDeviceToHost));
    if (out->stego && out->n) HIPCHK(c, hipMemcpy(out->stego, c->E.stego, out->n, hipMemcpyDeviceToHost));
    if (out->flip && out->n) HIPCHK(c, hipMemcpy(out->flip, c->d_flip, out->n, hipMemcpyDeviceToHost));
    if (out->message && m_copy) HIPCHK(c, hipMemcpy(out->message, c->E.message, m_copy, hipMemcpyDeviceToHost));
    return 0;
}

/* the embedding stage on the records that stand in the context's record buffer (F.rec_mb = E.mbs): what embed_pframe and embed_records share */
static int embed_stage(pcamv_ctx *c, float emrate, const uint8_t *message, int message_len, pcamv_embed_t *out)
{
    if (message) {
        if (message_len < 0 || message_len > c->cap) return fail(c, PCAMV_EINVAL, "message_len");
        HIPCHK(c, hipMemcpy(c->d_user_msg, message, message_len, hipMemcpyHostToDevice));
        c->E.user_message = c->d_user_msg; c->E.user_message_len = message_len;
    } else { c->E.user_message = NULL; c->E.user_message_len = 0; }
    c->E.emrate = emrate;
    TRY(ctx_launch(c, ST_EMBED));
    return fetch_embed(c, out);
}
/* is the context a member of a batch that has one message attached?  Its bits then come from that batch's steps alone */
static int ctx_under_message(pcamv_ctx *c, const char *call)
{
    for (int k = 0; k < c->n_member; k++)
        if (c->member_of[k]->d_msg) return fail(c, PCAMV_EINVAL, "%s: a batch of this context has a message attached (pcamv_gpu_batch_set_message)", call);
    return 0;
}
extern "C" int pcamv_gpu_embed_pframe(pcamv_ctx_t *c, float emrate, const uint8_t *message, int message_len, pcamv_embed_t *out)
{
    if (!c || !out || emrate <= 0) return PCAMV_EINVAL;
    if (!message) TRY(ctx_under_message(c, "embed_pframe without a message"));
    HIPCHK(c, hipSetDevice(c->device));
    return embed_stage(c, emrate, message, message_len, out);
}
/* The probe of the embedding stage: a caller's records take the place an analysis would have written them to, then the stage as
 * embed_pframe runs it.  Afterwards the context stands as after an analysis that produced them (final_mvs, batch_extract_step and
 * the writers' final motion read the record buffer and the new flip map). */
extern "C" int pcamv_gpu_embed_records(pcamv_ctx_t *c, const pcamv_mb_t *mbs, float emrate, const uint8_t *message, int message_len, pcamv_embed_t *out)
{
    if (!c || !mbs || !out || emrate <= 0) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());          /* work in flight (a receiver's launch on another stream) may still read the records */
    HIPCHK(c, hipMemcpy(c->F.rec_mb, mbs, (size_t)c->F.n_mb * sizeof(pcamv_mb_t), hipMemcpyHostToDevice));
    drop_rec_reuse(c);          /* the reconstruction planes hold no first pass of THESE records */
    return embed_stage(c, emrate, message, message_len, out);
}

/* the carrier MVs of a record in embedding order (encoder.c:1566-1647; the device's carrier_slots): their slots in mv[], and how many */
static int mb_carrier_slots(const pcamv_mb_t *mb, int slots[16])
{
    int n = 0;
    if (!mb->used) return 0;
    if (mb->i_type == PCAMV_P_8x8) {
        for (int i = 0; i < 4; i++)
            switch (mb->i_sub_partition[i]) {
            case PCAMV_D_L0_8x8: slots[n++] = i * 4; break;
            case PCAMV_D_L0_4x8: slots[n++] = i * 4; slots[n++] = i * 4 + 1; break;
            case PCAMV_D_L0_8x4: slots[n++] = i * 4; slots[n++] = i * 4 + 2; break;
            default: for (int j = 0; j < 4; j++) slots[n++] = i * 4 + j; break;
            }
    } else if (mb->i_type == PCAMV_P_L0) {
        slots[n++] = 0;
        if (mb->i_partition == PCAMV_D_8x16) slots[n++] = 4;
        else if (mb->i_partition == PCAMV_D_16x8) slots[n++] = 8;
    }
    return n;
}

/* Pass 2 of the frame last analysed: final MVs (the record with mv_stego where the flip map says so; the flip
 * map of the last embed_pframe when flips == NULL), reconstruction, loop filter.  out_final / recon /
 * deblocked may be NULL.  The deblocked picture stays on the device (the context's reconstruction planes) and
 * the final motion field becomes the one PCAMV_PREV_FIELD_INTERNAL hands to the next frame. */
extern "C" int pcamv_gpu_pass2_pframe(pcamv_ctx_t *c, const uint8_t *flips, int n_flips, pcamv_mb_t *out_final,
                                      uint8_t *const recon[3], uint8_t *const deblocked[3])
{
    if (!c) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_mb = (size_t)c->F.n_mb;
    if (flips) {
        if (n_flips < 0 || n_flips > c->cap) return fail(c, PCAMV_EINVAL, "n_flips");
        HIPCHK(c, hipMemset(c->d_flip_user, 0, (size_t)c->cap));
        if (n_flips) HIPCHK(c, hipMemcpy(c->d_flip_user, flips, n_flips, hipMemcpyHostToDevice));
        c->F.flip = c->d_flip_user; c->F.mbflip = nullptr;          /* a caller's map: the per-macroblock summary belongs to the embedding stage's own */
        /* carrier index of every macroblock from the record (the embedding stage may not have run) */
        HostTmp<pcamv_mb_t> h(n_mb);
        HostTmp<int> base(n_mb);
        if (!h || !base) return fail(c, PCAMV_ENOMEM, "pass2");
        HIPCHK(c, hipMemcpy(h, c->F.rec_mb, n_mb * sizeof(pcamv_mb_t), hipMemcpyDeviceToHost));
        int k = 0, slots[16];
        for (size_t xy = 0; xy < n_mb; xy++) { base[xy] = k; k += mb_carrier_slots(&h[xy], slots); }
        HIPCHK(c, hipMemcpy(c->E.car_base, base, n_mb * sizeof(int), hipMemcpyHostToDevice));
        if (k > n_flips) return fail(c, PCAMV_EINVAL, "flip map has %d entries, the record has %d carriers", n_flips, k);
    } else { c->F.flip = c->d_flip; c->F.mbflip = c->d_mbflip; }
    const size_t ysz = (size_t)c->F.w * c->F.h;
    /* pass-2 reconstruction first (for callers that want it before the loop filter), then the filter */
    pcamv_batch *b = c->self;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    pass2_takes_rec(c);
    {   /* pass 2 only */
        const FrameDev *dF; const EmbedDev *dE; int slot;
        TRY(on_behalf(c, b, batch_push_descs(b, c->stream, &dF, &dE, &slot)));
        const FrameDev &F = c->F;
        for (int pass = 0; pass < 2; pass++) {
            diag_launch(b->n_diag, F, [&](int cnt, int d) { pcamv_launch_pass2_diag(pass == 0 ? P2D_PASS2 : P2D_DEBLOCK, cnt, 1, c->stream, dF, d); });
            HIPCHK(c, hipStreamSynchronize(c->stream));
            uint8_t *const *dst = pass == 0 ? recon : deblocked;
            if (dst)
                for (int i = 0; i < 3; i++)
                    if (dst[i]) HIPCHK(c, hipMemcpy(dst[i], c->F.rec[i], i ? ysz / 4 : ysz, hipMemcpyDeviceToHost));
        }
        TRY(on_behalf(c, b, ring_release(b, b->ring, slot, c->stream)));
    }
    if (out_final) {
        HIPCHK(c, hipMemcpy(out_final, c->F.rec_mb, n_mb * sizeof(pcamv_mb_t), hipMemcpyDeviceToHost));
        HostTmp<int16_t> mv(n_mb * 32);
        if (!mv) return fail(c, PCAMV_ENOMEM, "pass2");
        HIPCHK(c, hipMemcpy(mv, c->F.mv, n_mb * 64, hipMemcpyDeviceToHost));
        const int s4 = 4 * c->F.mb_w;
        static const int bx[16] = {0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3}, by[16] = {0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3};
        for (int xy = 0; xy < c->F.n_mb; xy++) {
            const int mx = xy % c->F.mb_w, my = xy / c->F.mb_w;
            for (int i = 0; i < 16; i++) {
                const int16_t *s = mv + 2 * ((4 * my + by[i]) * s4 + 4 * mx + bx[i]);
                out_final[xy].mv[i][0] = s[0]; out_final[xy].mv[i][1] = s[1]; out_final[xy].ref[i] = 0;
            }
        }
    }
    return 0;
}

/* ---- a QP per context on the device (pcamv_rate.h, k_frame_qp) */
/* The batch's tables for device QPs lo .. hi: the MV cost tables and (--subme >= 6) the slice-start context states of the QPs allowed
 * only (a rate's qp_min .. qp_max; 0 .. 51 for a caller's array), built by the functions the per-context tables come from, and per
 * distinct (chroma offset, deadzones) among the contexts 52 rows taken out of a descriptor that pcamv_frame_set_qp and the two pointers
 * were written into -- what frame_use_qp does.  The row of a QP outside lo .. hi, which nothing allowed selects, points at the tables of
 * the nearest QP inside, so that no row holds a pointer to nothing.  Allocates and copies: the first device-QP step or rate_open of a
 * batch pays for it, and so does one that allows QPs the tables do not hold yet -- they are made again for the union, behind a
 * synchronisation, and the contexts that read the old rows are pointed at the new ones */
static int qp_tables_setup(pcamv_batch *b, int lo, int hi)
{
    if (b->d_qp_rows && b->qp_lo <= lo && hi <= b->qp_hi) return 0;
    if (b->d_qp_rows) { lo = lo < b->qp_lo ? lo : b->qp_lo; hi = hi > b->qp_hi ? hi : b->qp_hi; }
    const size_t held = (size_t)(hi - lo + 1);
    const size_t cost_stride = (size_t)PCAMV_COST_MV_LEN + 1, cabac_stride = ((size_t)PCAMV_CHAIN_BYTES + 255) & ~(size_t)255;
    static_assert((PCAMV_COST_MV_LEN + 1) % 2 == 0, "prim_mv_cost fetches the dword that holds an entry: every QP's table starts on one");
    std::vector<int> of((size_t)b->n), first;
    for (int i = 0; i < b->n; i++) {
        const pcamv_params_t &p = b->ctx[i]->p;
        size_t t = 0;
        for (; t < first.size(); t++) {
            const pcamv_params_t &q = b->ctx[first[t]]->p;
            if (q.i_chroma_qp_offset == p.i_chroma_qp_offset && q.i_luma_deadzone[0] == p.i_luma_deadzone[0] && q.i_luma_deadzone[1] == p.i_luma_deadzone[1]) break;
        }
        if (t == first.size()) first.push_back(i);
        of[(size_t)i] = (int)t;
    }
    if (first.size() > PCAMV_QP_TABLES_MAX)
        return fail(b, PCAMV_EUNSUP, "the batch's contexts have %zu distinct (chroma offset, deadzones): at most %d row tables are kept", first.size(), PCAMV_QP_TABLES_MAX);
    HostTmp<int16_t> h_cost(held * cost_stride);
    HostTmp<uint8_t> h_cabac(held * cabac_stride);
    HostTmp<uint32_t> h_rows(first.size() * QPROW_QPS * QPROW_DWORDS);
    if (!h_cost || !h_cabac || !h_rows) return fail(b, PCAMV_ENOMEM, "the tables of QPs %d .. %d", lo, hi);
    memset(h_cost, 0, held * cost_stride * sizeof(int16_t)); memset(h_cabac, 0, held * cabac_stride);
    DevBuf<int16_t> d_cost; DevBuf<uint8_t> d_cabac; DevBuf<uint32_t> d_rows;
    TRY(d_cost.room(b, held * cost_stride)); TRY(d_rows.room(b, first.size() * QPROW_QPS * QPROW_DWORDS));
    if (b->b_mbrd) TRY(d_cabac.room(b, held * cabac_stride));
    for (int qp = lo; qp <= hi; qp++) {
        pcamv_build_cost_mv(qp, h_cost + (size_t)(qp - lo) * cost_stride);
        if (b->b_mbrd) pcamv_build_cabac_init(qp, h_cabac + (size_t)(qp - lo) * cabac_stride);
    }
    for (int qp = 0; qp < QPROW_QPS; qp++) {
        const size_t at = (size_t)((qp < lo ? lo : qp > hi ? hi : qp) - lo);       /* (the tables of this QP, or of the nearest one held) */
        for (size_t t = 0; t < first.size(); t++) {
            const pcamv_ctx *c = b->ctx[first[t]];
            FrameDev F = c->F;
            pcamv_frame_set_qp(&F, &c->p, qp);
            F.cost_mv = d_cost + at * cost_stride + PCAMV_COST_MV_CENTRE;
            if (F.b_mbrd) F.cabac_init = d_cabac + at * cabac_stride;
            qprow_take(&F, h_rows + (t * QPROW_QPS + (size_t)qp) * QPROW_DWORDS);
        }
    }
    HIPCHK(b, hipMemcpy(d_cost, h_cost, held * cost_stride * sizeof(int16_t), hipMemcpyHostToDevice));
    if (b->b_mbrd) HIPCHK(b, hipMemcpy(d_cabac, h_cabac, held * cabac_stride, hipMemcpyHostToDevice));
    HIPCHK(b, hipMemcpy(d_rows, h_rows, first.size() * QPROW_QPS * QPROW_DWORDS * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (b->d_qp_rows) HIPCHK(b, hipDeviceSynchronize());      /* (the tables before these are freed on return: work in flight may still read them) */
    std::swap(b->d_qp_cost.p, d_cost.p); std::swap(b->d_qp_cost.cap, d_cost.cap);
    std::swap(b->d_qp_cabac.p, d_cabac.p); std::swap(b->d_qp_cabac.cap, d_cabac.cap);
    std::swap(b->d_qp_rows.p, d_rows.p); std::swap(b->d_qp_rows.cap, d_rows.cap);
    b->qp_table_of.swap(of);
    b->qp_lo = lo; b->qp_hi = hi;
    for (int i = 0; i < b->n; i++)
        if (b->ctx[i]->qp_owner == b && b->ctx[i]->qp_rows) b->ctx[i]->qp_rows = b->d_qp_rows + (size_t)b->qp_table_of[(size_t)i] * QPROW_QPS * QPROW_DWORDS;
    return 0;
}
/* What context i of the batch needs before it can take its QP from its device cell: the cell (zeros), and a host descriptor that holds
 * what its last host QP left -- QP 26 where there was none, so that it never holds a table pointer that is NULL.  Changes no mode */
static int qp_device_prepare(pcamv_batch *b, int i)
{
    pcamv_ctx *c = b->ctx[i];
    if (!c->d_qp_cell) { const int rc = ctx_alloc(c, &c->d_qp_cell, 2, 0); if (rc) return fail(b, rc, "%s", c->err); }
    if (!c->F.cost_mv) {
        const uint32_t *rows = c->qp_rows; pcamv_batch *owner = c->qp_owner;
        const int rc = ensure_qp(c, 26);
        c->qp_rows = rows; c->qp_owner = owner;
        if (rc) return fail(b, rc, "%s", c->err);
    }
    return 0;
}
/* ... and from here on (until ensure_qp) it does */
static void qp_device_enter(pcamv_batch *b, int i)
{
    pcamv_ctx *c = b->ctx[i];
    c->qp_rows = b->d_qp_rows + (size_t)b->qp_table_of[(size_t)i] * QPROW_QPS * QPROW_DWORDS; c->qp_owner = b;
}

/* one step of every context of the batch on resident inputs: plane production + analysis + embedding.  The QPs: qps[i] (host), else
 * d_qp[i] (device, borrowed for the call; its values lie within lo .. hi or are clamped to 0 .. 51), else qp_all.  A device-QP step
 * changes the contexts' mode only once nothing of its preparation can fail any more, and puts it back if its launches fail: no context
 * is left reading a cell that no step has written */
static int batch_step_at(pcamv_batch_t *b, int qp_all, const int32_t *qps, const int32_t *d_qp, float emrate, void *stream, int lo = 0, int hi = QPROW_QPS - 1)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    if (qps) for (int i = 0; i < b->n; i++) if (qps[i] < 0 || qps[i] > 51) return fail(b, PCAMV_EINVAL, "qp %d of context %d out of range", qps[i], i);
    if (d_qp) TRY(qp_tables_setup(b, lo, hi));
    for (int i = 0; d_qp && i < b->n; i++) {
        TRY(qp_device_prepare(b, i));
        if (!b->ctx[i]->F.raw[0]) return fail(b, PCAMV_EINVAL, "context %d has no reference", i);
    }
    std::vector<std::pair<const uint32_t *, pcamv_batch *>> was;
    for (int i = 0; d_qp && i < b->n; i++) was.push_back({b->ctx[i]->qp_rows, b->ctx[i]->qp_owner});
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        if (d_qp) qp_device_enter(b, i);
        else {
            int rc = ensure_qp(c, qps ? qps[i] : qp_all);
            if (rc) return fail(b, rc, "%s", c->err);
        }
        if (!c->F.raw[0]) return fail(b, PCAMV_EINVAL, "context %d has no reference", i);
        c->F.embed = emrate > 0; c->E.emrate = emrate; c->E.user_message = NULL; c->E.user_message_len = 0;
        c->F.flip = c->d_flip; c->F.mbflip = c->d_mbflip;        /* a closed-loop step applies the flip map of its own embedding stage, never a caller's map left by pass2_pframe */
    }
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    b->qp_src = d_qp;           /* (the step's own push takes the caller's values into the cells; later pushes read the cells) */
    const int rc = batch_launch(b, ST_PLANES | ST_ANALYSE | (emrate > 0 ? ST_EMBED : 0) | (b->closed_loop ? ST_PASS2 : 0), st);
    b->qp_src = NULL;
    if (rc) for (size_t i = 0; i < was.size(); i++) { b->ctx[i]->qp_rows = was[i].first; b->ctx[i]->qp_owner = was[i].second; }
    return rc;
}
extern "C" int pcamv_gpu_batch_step(pcamv_batch_t *b, int qp, float emrate, void *stream) { return batch_step_at(b, qp, NULL, NULL, emrate, stream); }
extern "C" int pcamv_gpu_batch_step_qps(pcamv_batch_t *b, const int32_t *qp, float emrate, void *stream)
{
    if (!b || !qp) return PCAMV_EINVAL;
    return batch_step_at(b, 0, qp, NULL, emrate, stream);
}
extern "C" int pcamv_gpu_batch_step_qp_device(pcamv_batch_t *b, const int32_t *d_qp, float emrate, void *stream)
{
    if (!b || !d_qp) return PCAMV_EINVAL;
    return batch_step_at(b, 0, NULL, d_qp, emrate, stream);
}
/* synchronises: word `w` of every context's cell (0: the QP in force, 1: the status of the step that set it), `none` where no QP is in force */
static int qp_cells_fetch(pcamv_batch *b, int w, int none, int32_t *out)
{
    if (!b || !out) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    HIPCHK(b, hipDeviceSynchronize());
    for (int i = 0; i < b->n; i++) {
        out[i] = none;
        if (b->ctx[i]->qp_rows) HIPCHK(b, hipMemcpy(&out[i], b->ctx[i]->d_qp_cell + w, sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}
extern "C" int pcamv_gpu_batch_qp_status(pcamv_batch_t *b, int32_t *status) { return qp_cells_fetch(b, 1, 0, status); }
extern "C" int pcamv_gpu_batch_qps(pcamv_batch_t *b, int32_t *qp) { return qp_cells_fetch(b, 0, -1, qp); }
extern "C" int pcamv_gpu_qp_device(pcamv_ctx_t *c, int32_t *qp)
{
    if (!c || !qp) return PCAMV_EINVAL;
    return on_behalf(c, c->self, qp_cells_fetch(c->self, 0, -1, qp));
}

/* ---- the rate controller (pcamv_rate.h: pcamv_rate_step is the rule; k_rate_update) */
extern "C" int pcamv_gpu_rate_update(const pcamv_rate_params_t *params, pcamv_rate_state_t *state, int64_t len, int32_t write_status, int32_t *d)
{
    if (!params || !state || !pcamv_rate_params_ok(params)) return PCAMV_EINVAL;
    const int step = pcamv_rate_step(params, state, (long long)len, write_status);
    if (d) *d = step;
    return 0;
}
extern "C" int pcamv_gpu_rate_update_device(pcamv_ctx_t *c, const pcamv_rate_params_t *params, pcamv_rate_state_t *states, const int64_t *len,
                                            const int32_t *write_status, int n, int32_t *d)
{
    if (!c || !params || !states || !len || !write_status || !d || n < 1 || n > (1 << 24)) return PCAMV_EINVAL;
    for (int i = 0; i < n; i++) if (!pcamv_rate_params_ok(&params[i])) return fail(c, PCAMV_EINVAL, "rate_update_device: the parameters of case %d are out of range", i);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<pcamv_rate_params_t> d_p; DevBuf<pcamv_rate_state_t> d_s; DevBuf<long long> d_len; DevBuf<int> d_int;
    TRY(d_p.room(c, (size_t)n)); TRY(d_s.room(c, (size_t)n)); TRY(d_len.room(c, (size_t)n)); TRY(d_int.room(c, 2 * (size_t)n));
    HIPCHK(c, hipMemcpy(d_p, params, sizeof(*params) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_s, states, sizeof(*states) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_len, len, 8 * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_int, write_status, 4 * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(d_int + n, 0xA5, 4 * (size_t)n));
    hipLaunchKernelGGL(k_rate_cases, dim3((n + 63) / 64), dim3(64), 0, c->stream, (const pcamv_rate_params_t *)d_p, d_s.p, (const long long *)d_len, (const int *)d_int, n, d_int + n);
    TRY(launched(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(states, d_s, sizeof(*states) * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(d, d_int + n, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}
/* the launch of k_rate_update over the batch's streams as they stand on `st`: behind an open, or behind a k_stream_commit */
static void rate_launch(pcamv_batch *b, int open, hipStream_t st)
{
    RateJobs J;
    J.P = b->rate; J.state = b->d_rate; J.qp = b->d_rate_qp; J.ctx = (const SwsCtx *)b->so.d_own.p; J.status = b->d_wstat; J.n = b->n; J.open = open;
    timed_kernel(b, KT_RATE_UPDATE, st, k_rate_update, dim3((b->n + 63) / 64), dim3(64), J);
}
extern "C" int pcamv_gpu_batch_rate_open(pcamv_batch_t *b, const pcamv_rate_params_t *params, void *stream)
{
    if (!b || !params) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    if (!pcamv_rate_params_ok(params))
        return fail(b, PCAMV_EINVAL, "rate_open: target_bits 1 .. 2^40, 0 <= qp_min <= qp_init <= qp_max <= 51, max_step 1 .. 6, window 1 .. 1024");
    if (!b->so.ready) return fail(b, PCAMV_EINVAL, "rate_open: no byte streams were opened on this batch yet (pcamv_gpu_batch_stream_open)");
    if (b->rate_open) HIPCHK(b, hipDeviceSynchronize());       /* (a re-open: the states are written again, and work in flight may still read them) */
    b->rate_open = 0;
    TRY(qp_tables_setup(b, params->qp_min, params->qp_max));
    TRY(b->d_rate.room(b, (size_t)b->n)); TRY(b->d_rate_qp.room(b, (size_t)b->n));
    if (!b->d_wstat) TRY(b->d_wstat.room(b, (size_t)b->n));
    b->rate = *params;
    rate_launch(b, 1, stream ? (hipStream_t)stream : b->ctx[0]->stream);
    TRY(launched(b));
    b->rate_open = 1;
    return 0;
}
extern "C" int pcamv_gpu_batch_rate_close(pcamv_batch_t *b)
{
    if (!b) return PCAMV_EINVAL;
    if (!b->rate_open) return fail(b, PCAMV_EINVAL, "rate_close: no rate is open on this batch");
    b->rate_open = 0;           /* (the states stay where they are: steps in flight read the cells) */
    return 0;
}
extern "C" int pcamv_gpu_batch_step_rate(pcamv_batch_t *b, float emrate, void *stream)
{
    if (!b) return PCAMV_EINVAL;
    if (!b->rate_open) return fail(b, PCAMV_EINVAL, "step_rate: no rate is open on this batch (pcamv_gpu_batch_rate_open)");
    return batch_step_at(b, 0, NULL, b->d_rate_qp, emrate, stream, b->rate.qp_min, b->rate.qp_max);
}
/* synchronises */
extern "C" int pcamv_gpu_batch_rate_tell(pcamv_batch_t *b, pcamv_rate_state_t *states)
{
    if (!b || !states) return PCAMV_EINVAL;
    if (!b->rate_open) return fail(b, PCAMV_EINVAL, "rate_tell: no rate is open on this batch");
    HIPCHK(b, hipSetDevice(b->device));
    HIPCHK(b, hipDeviceSynchronize());
    HIPCHK(b, hipMemcpy(states, b->d_rate, sizeof(*states) * (size_t)b->n, hipMemcpyDeviceToHost));
    return 0;
}
/* ---- the source feed (pcamv_source.h, k_source_feed) */
extern "C" int pcamv_gpu_source_check(const pcamv_source_t *src, size_t clip_bytes, int mb_w, int mb_h, int64_t *n_pictures)
{
    long long n = 0;
    if (n_pictures) *n_pictures = 0;
    if (clip_bytes > ((size_t)1 << 62)) return PCAMV_EINVAL;
    const int rc = src_check(src, (long long)clip_bytes, mb_w, mb_h, &n);
    if (!rc && n_pictures) *n_pictures = n;
    return rc;
}
extern "C" int pcamv_gpu_source_picture(const pcamv_source_t *src, const uint8_t *clip, size_t clip_bytes, int64_t picture, int mb_w, int mb_h, uint8_t *const out[3])
{
    int64_t n = 0;
    if (!clip || !out || !out[0] || !out[1] || !out[2]) return PCAMV_EINVAL;
    TRY(pcamv_gpu_source_check(src, clip_bytes, mb_w, mb_h, &n));
    if (picture < 0 || picture >= n) return PCAMV_EINVAL;
    src_picture_naive(src, clip + picture * src->picture_stride, mb_w, mb_h, out);
    return 0;
}
extern "C" int pcamv_gpu_upload_picture(pcamv_ctx_t *c, const pcamv_source_t *src, const uint8_t *clip, size_t clip_bytes, int64_t picture)
{
    if (!c || !src || !clip) return PCAMV_EINVAL;
    const size_t ysz = (size_t)c->F.w * c->F.h;
    HostTmp<uint8_t> tmp(ysz + ysz / 2);
    if (!tmp) return fail(c, PCAMV_ENOMEM, "upload_picture: the staging planes");
    uint8_t *const out[3] = {tmp, tmp + ysz, tmp + ysz + ysz / 4};
    if (pcamv_gpu_source_picture(src, clip, clip_bytes, picture, c->F.mb_w, c->F.mb_h, out))
        return fail(c, PCAMV_EINVAL, "upload_picture: the source does not describe pictures of this context's %d x %d macroblocks, or picture %lld is not inside the clip",
                    c->F.mb_w, c->F.mb_h, (long long)picture);
    const int stride[3] = {c->F.w, c->F.w / 2, c->F.w / 2};
    return pcamv_gpu_upload_fenc(c, out, stride);
}
extern "C" int pcamv_gpu_batch_feed_device(pcamv_batch_t *b, const void *d_clip, int64_t clip_bytes, const pcamv_source_t *src, const int64_t *d_picture, void *stream)
{
    if (!b || !d_clip || !src || !d_picture) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    const FrameDev &F = b->ctx[0]->F;
    SrcFeed J;
    J.S = *src; J.clip = (const uint8_t *)d_clip; J.picture = (const long long *)d_picture; J.mb_w = F.mb_w; J.mb_h = F.mb_h; J.n = b->n;
    if (clip_bytes < 0 || src_check(src, clip_bytes, F.mb_w, F.mb_h, &J.n_pictures))
        return fail(b, PCAMV_EINVAL, "feed: the source does not describe pictures of %d x %d macroblocks (even sizes inside the last macroblock, pitches of a line at least, offsets >= 0)", F.mb_w, F.mb_h);
    const long long blocks = (long long)b->n * src_items(F.mb_h);
    if (blocks >= (1LL << 26)) return fail(b, PCAMV_EUNSUP, "feed: %lld work items in one launch (a launch of 64-lane blocks holds fewer than 2^26)", blocks);
    if (!b->d_src_planes) {         /* once for good: the planes are the contexts' own from open to close */
        std::vector<uint8_t *> h((size_t)b->n * 3);
        for (int i = 0; i < b->n; i++) for (int k = 0; k < 3; k++) h[(size_t)i * 3 + k] = b->ctx[i]->d_fenc[k];
        TRY(b->d_src_status.room(b, (size_t)b->n));
        HIPCHK(b, hipMemset(b->d_src_status, 0, sizeof(int) * (size_t)b->n));
        DevBuf<uint8_t *> d; TRY(d.room(b, h.size()));
        HIPCHK(b, hipMemcpy(d, h.data(), sizeof(uint8_t *) * h.size(), hipMemcpyHostToDevice));
        std::swap(b->d_src_planes.p, d.p); std::swap(b->d_src_planes.cap, d.cap);
    }
    J.planes = b->d_src_planes; J.status = b->d_src_status;
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    timed_kernel(b, KT_SOURCE_FEED, st, k_source_feed, dim3((unsigned)blocks), dim3(64), J);
    TRY(launched(b));
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        for (int k = 0; k < 3; k++) c->F.fenc[k] = c->d_fenc[k];
        drop_rec_reuse(c);          /* a new source: a second pass re-encodes every macroblock on it */
    }
    return 0;
}
/* synchronises */
extern "C" int pcamv_gpu_batch_feed_status(pcamv_batch_t *b, int32_t *status)
{
    if (!b || !status) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    HIPCHK(b, hipDeviceSynchronize());
    if (!b->d_src_status) { memset(status, 0, sizeof(int32_t) * (size_t)b->n); return 0; }
    HIPCHK(b, hipMemcpy(status, b->d_src_status, sizeof(int32_t) * (size_t)b->n, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int pcamv_gpu_debug_fetch_fenc(pcamv_ctx_t *c, uint8_t *const out[3], int *guard_intact)
{
    if (!c || !out || !out[0] || !out[1] || !out[2]) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const size_t ysz = (size_t)c->F.w * c->F.h;
    int intact = 1;
    for (int i = 0; i < 3; i++) {
        const size_t sz = i ? ysz / 4 : ysz;
        uint8_t g[PCAMV_SRC_GUARD];
        HIPCHK(c, hipMemcpy(out[i], c->d_fenc[i], sz, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(g, c->d_fenc[i] + sz, PCAMV_SRC_GUARD, hipMemcpyDeviceToHost));
        for (int k = 0; k < PCAMV_SRC_GUARD; k++) if (g[k] != SRC_GUARD_BYTE) intact = 0;
    }
    if (guard_intact) *guard_intact = intact;
    return 0;
}

extern "C" int pcamv_gpu_step_device(pcamv_ctx_t *c, int qp, float emrate, void *stream)
{
    if (!c) return PCAMV_EINVAL;
    TRY(ctx_under_message(c, "step_device"));
    return on_behalf(c, c->self, pcamv_gpu_batch_step(c->self, qp, emrate, stream ? stream : (void *)c->stream));
}
extern "C" int pcamv_gpu_fetch_results(pcamv_ctx_t *c, pcamv_mb_t *out_mb, pcamv_embed_t *out)
{
    if (!c) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    TRY(on_behalf(c, c->last, flow_check(c->last)));
    if (out_mb) HIPCHK(c, hipMemcpy(out_mb, c->F.rec_mb, (size_t)c->F.n_mb * sizeof(pcamv_mb_t), hipMemcpyDeviceToHost));
    if (out) return fetch_embed(c, out);
    return 0;
}

/* ------------------------------------------------------------------ payload path
 * Sender: a payload attached to a context is what its frames embed wherever no caller's message is given (embed_pframe(NULL),
 * step_device, batch_step in open and closed loop) -- the reference draws those bits from rand() (encoder.c:1838-1840); the cursor
 * lives on the device and moves by each frame's m there, so closed-loop steps need no host round trip. */
static int payload_attach(pcamv_ctx *c, const uint8_t *d_bytes, int64_t n_bits)
{
    c->E.payload = n_bits > 0 ? d_bytes : NULL; c->E.payload_bits = n_bits > 0 ? n_bits : 0;
    c->X.payload = c->E.payload; c->X.payload_bits = c->E.payload_bits;
    HIPCHK(c, hipMemset(c->E.pstate + PST_TX, 0, sizeof(long long)));
    return 0;
}
extern "C" int pcamv_gpu_set_payload(pcamv_ctx_t *c, const uint8_t *bytes, int64_t n_bits)
{
    if (!c || n_bits < 0 || (n_bits > 0 && !bytes)) return PCAMV_EINVAL;
    TRY(ctx_under_message(c, "set_payload"));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());          /* frames in flight still read the payload attached so far */
    const size_t nb = bytes ? (size_t)((n_bits + 7) >> 3) : 0;
    if (nb > c->payload_own_bytes) {
        ctx_free(c, &c->d_payload_own); c->payload_own_bytes = 0;
        TRY(ctx_alloc(c, &c->d_payload_own, nb));
        c->payload_own_bytes = nb;
    }
    if (nb) HIPCHK(c, hipMemcpy(c->d_payload_own, bytes, nb, hipMemcpyHostToDevice));
    return payload_attach(c, nb ? c->d_payload_own : NULL, nb ? n_bits : 0);
}
extern "C" int pcamv_gpu_set_payload_device(pcamv_ctx_t *c, const void *d_bytes, int64_t n_bits)
{
    if (!c || n_bits < 0 || (n_bits > 0 && !d_bytes)) return PCAMV_EINVAL;
    TRY(ctx_under_message(c, "set_payload_device"));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    return payload_attach(c, d_bytes ? (const uint8_t *)d_bytes : NULL, d_bytes ? n_bits : 0);
}
/* after a synchronisation: did a frame run past the reserved received buffer?  (reported once, like flow_check) */
static int rx_check(pcamv_ctx *c, long long *pstate_out)
{
    long long st[PST_WORDS];
    HIPCHK(c, hipMemcpy(st, c->E.pstate, sizeof(st), hipMemcpyDeviceToHost));
    if (pstate_out) memcpy(pstate_out, st, sizeof(st));
    if (st[PST_OVERRUN]) {
        hipMemset(c->E.pstate + PST_OVERRUN, 0, sizeof(long long));
        return fail(c, PCAMV_ENOMEM, "received stream: %lld bits extracted, %lld reserved (the bits beyond were dropped)", st[PST_RX], c->X.rx_cap_bits);
    }
    return 0;
}
extern "C" int pcamv_gpu_payload_tell(pcamv_ctx_t *c, int64_t *consumed_bits, int64_t *payload_bits)
{
    if (!c) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    long long tx = 0;
    HIPCHK(c, hipMemcpy(&tx, c->E.pstate + PST_TX, sizeof(tx), hipMemcpyDeviceToHost));
    if (consumed_bits) *consumed_bits = tx;
    if (payload_bits) *payload_bits = c->E.payload_bits;
    return 0;
}

/* Receiver.  rx_reserve: room for n_bits of received stream (0 releases it) and the per-frame scratch; the stream starts empty, the
 * receiver's column generator at its initial state. */
static int rx_scratch(pcamv_ctx *c)
{
    if (c->X.stego) return 0;
    TRY(ctx_alloc(c, &c->X.stego, (size_t)c->cap)); TRY(ctx_alloc(c, &c->d_rx_bits, (size_t)c->cap));
    TRY(ctx_alloc(c, &c->X.hdr, 8, 0)); TRY(ctx_alloc(c, &c->X.cols, 2 * STC_MAXW));
    return 0;
}
/* the records of the receiving side that do not come from an analysis (host records, parsed slices), with a guard behind them */
static int rx_mbs(pcamv_ctx *c)
{
    if (c->d_rx_mbs) return 0;
    TRY(ctx_alloc(c, &c->d_rx_mbs, (size_t)c->F.n_mb + SLICE_GUARD_MBS));
    HIPCHK(c, hipMemset(c->d_rx_mbs + c->F.n_mb, 0xA5, SLICE_GUARD_MBS * sizeof(pcamv_mb_t)));
    return 0;
}
extern "C" int pcamv_gpu_rx_reset(pcamv_ctx_t *c)
{
    if (!c) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const long long st[3] = {0, 0, 1};          /* PST_RX, PST_OVERRUN, PST_RX_LCG */
    HIPCHK(c, hipMemcpy(c->E.pstate + PST_RX, st, sizeof(st), hipMemcpyHostToDevice));
    if (c->d_rx) HIPCHK(c, hipMemset(c->d_rx, 0, (size_t)((c->X.rx_cap_bits + 31) >> 5) * 4));
    return 0;
}
extern "C" int pcamv_gpu_rx_reserve(pcamv_ctx_t *c, int64_t n_bits)
{
    if (!c || n_bits < 0) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    ctx_free(c, &c->d_rx); c->X.rx = NULL; c->X.rx_cap_bits = 0;
    if (n_bits) {
        TRY(rx_scratch(c));
        TRY(ctx_alloc(c, &c->d_rx, (size_t)((n_bits + 31) >> 5)));
        c->X.rx = c->d_rx; c->X.rx_cap_bits = n_bits;
    }
    return pcamv_gpu_rx_reset(c);
}
extern "C" int pcamv_gpu_rx_tell(pcamv_ctx_t *c, int64_t *received_bits, int64_t *reserved_bits)
{
    if (!c) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    long long st[PST_WORDS];
    const int rc = rx_check(c, st);
    if (received_bits) *received_bits = st[PST_RX];
    if (reserved_bits) *reserved_bits = c->X.rx_cap_bits;
    return rc;
}
extern "C" int pcamv_gpu_rx_fetch(pcamv_ctx_t *c, uint8_t *bytes, int64_t n_bits)
{
    if (!c || !bytes || n_bits < 0 || n_bits > c->X.rx_cap_bits) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    TRY(rx_check(c, NULL));
    if (n_bits) HIPCHK(c, hipMemcpy(bytes, c->d_rx, (size_t)((n_bits + 7) >> 3), hipMemcpyDeviceToHost));
    return 0;
}

/* k_extract_bits for nx frames whose descriptors are at dX; emrate bounds the message bits of a frame */
static void extract_bits_launch(pcamv_batch *b, const ExtractDev *dX, int nx, int cap, float emrate, hipStream_t st)
{
    /* workgroups per frame: enough for the most bits a frame of this rate can hold (+ the 63 positions in front of a frame's first
     * bit); the kernel strides if a frame has more (it cannot) */
    double most = emrate > 1.0f ? (double)(int)emrate : ceil((double)emrate * cap) + 1;
    if (most > cap) most = cap;
    const int groups = (int)((most + 63 + 255) / 256) > 0 ? (int)((most + 63 + 255) / 256) : 1;
    timed(b, KT_EXTRACT_BITS, st, [&] {
        for (int x0 = 0; x0 < nx; x0 += 65535)     /* (a grid's second dimension ends there: a window of many contexts has more frames) */
            hipLaunchKernelGGL(k_extract_bits, dim3(groups, nx - x0 < 65535 ? nx - x0 : 65535), dim3(256), 0, st, dX + x0);
    });
}
/* Under a batch reservation (one message for the batch): behind k_extract_count, the frames of a call of k slots per context get their
 * places in the batch's stream from one plan over all of them, then the chain with those places.  first: the codes of a stream call's
 * first stages (or NULL) */
static void extract_message_chain_launch(pcamv_batch *b, const ExtractDev *dX, int k, const int *first, hipStream_t st)
{
    const int jobs = b->n * k;
    int *m = b->d_mrx_job, *status = b->d_mrx_job + (size_t)b->n * PCAMV_STREAM_WINDOW_MAX;
    timed_kernel(b, KT_MESSAGE_JOBS, st, k_message_jobs, dim3((jobs + 255) / 256), dim3(256), dX, first, jobs, m, status);
    timed_kernel(b, KT_MESSAGE_PLAN, st, k_message_plan, dim3(1), dim3(MSG_PLAN_THREADS), m, status, b->n, k, b->mrx_bits, b->d_mrx_state, b->d_mrx_at, (const EmbedDev *)NULL);
    timed_kernel(b, KT_EXTRACT_CHAIN_MESSAGE, st, k_extract_chain_message, dim3((b->n + 63) / 64), dim3(64), dX, b->n, k, status, b->d_mrx_at);
}
/* the two kernels of the receiving side for nx frames (with a batch reservation: the frames of the batch's contexts, a window of one) */
static void extract_launch(pcamv_batch *b, const ExtractDev *dX, int nx, int cap, float emrate, hipStream_t st, const int *first = NULL)
{
    if (b->d_mrx) {
        timed_kernel(b, KT_EXTRACT_COUNT, st, k_extract_count, dim3(nx), dim3(1024), dX);
        extract_message_chain_launch(b, dX, 1, first, st);
    } else timed_kernel(b, KT_EXTRACT_PREPARE, st, k_extract_prepare, dim3(nx), dim3(1024), dX);
    extract_bits_launch(b, dX, nx, cap, emrate, st);
}
/* descriptors of the batch's contexts as they stand, into the next slot of the receiving side's ring */
static int batch_push_xdescs(pcamv_batch *b, hipStream_t st, const ExtractDev **dX, int *slot_out)
{
    if (!b->d_chk) {            /* (a batch's first extraction: made once, never regrown) */
        TRY(b->h_X.room(b, (size_t)b->n * NRING)); TRY(b->d_X.room(b, (size_t)b->n * NRING)); TRY(b->d_chk.room(b, (size_t)b->n));
    }
    int slot;
    TRY(ring_take(b, b->xring, &slot));
    ExtractDev *hX = b->h_X + (size_t)slot * b->n;
    for (int i = 0; i < b->n; i++) hX[i] = b->ctx[i]->X;
    if (b->d_mrx) for (int i = 0; i < b->n; i++) { hX[i].rx = b->d_mrx; hX[i].rx_cap_bits = b->mrx_bits; }      /* a batch reservation: every frame writes into the batch's stream */
    HIPCHK(b, hipMemcpyAsync(b->d_X + (size_t)slot * b->n, hX, sizeof(ExtractDev) * b->n, hipMemcpyHostToDevice, st));
    *dX = b->d_X + (size_t)slot * b->n; *slot_out = slot;
    return 0;
}
/* Every context's last step -- its records and the flip map of its embedding stage, both still on the device -- through the
 * receiving side, on `stream`, without a host synchronisation: between two closed-loop steps, or after the last one. */
extern "C" int pcamv_gpu_batch_extract_step(pcamv_batch_t *b, float emrate, void *stream)
{
    if (!b || emrate <= 0) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        if (!c->d_rx && !b->d_mrx) return fail(b, PCAMV_EINVAL, "context %d has no received buffer (pcamv_gpu_rx_reserve)", i);
        if (b->d_mrx) { const int rc_c = rx_scratch(c); if (rc_c) return fail(b, rc_c, "context %d: %s", i, c->err); }
        c->X.mbs = c->F.rec_mb; c->X.flip = c->d_flip; c->X.bits = NULL; c->X.emrate = emrate; c->X.slice_status = NULL;
    }
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    const ExtractDev *dX; int slot;
    TRY(batch_push_xdescs(b, st, &dX, &slot));
    extract_launch(b, dX, b->n, b->ctx[0]->cap, emrate, st);
    TRY(launched(b));
    return ring_release(b, b->xring, slot, st);
}
/* One frame from host records holding FINAL motion (what pcamv_gpu_parse_pslice_* reads out of a stream): uploaded, then the same
 * kernels.  bits_out (optional, 16 * mb_count bytes) receives the frame's message bits, one per byte; n / m its carriers and bits.
 * With a received buffer reserved the bits are appended to it as well. */
extern "C" int pcamv_gpu_extract_pframe(pcamv_ctx_t *c, const pcamv_mb_t *mbs, float emrate, uint8_t *bits_out, int32_t *n_out, int32_t *m_out)
{
    if (!c || !mbs || emrate <= 0) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    TRY(rx_scratch(c));
    TRY(rx_mbs(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_rx_mbs, mbs, (size_t)c->F.n_mb * sizeof(pcamv_mb_t), hipMemcpyHostToDevice));
    c->X.mbs = c->d_rx_mbs; c->X.flip = NULL; c->X.bits = c->d_rx_bits; c->X.emrate = emrate; c->X.slice_status = NULL;
    pcamv_batch *b = c->self;
    const ExtractDev *dX; int slot;
    TRY(on_behalf(c, b, batch_push_xdescs(b, c->stream, &dX, &slot)));
    extract_launch(b, dX, 1, c->cap, emrate, c->stream);
    TRY(launched(c));
    TRY(on_behalf(c, b, ring_release(b, b->xring, slot, c->stream)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int hdr[8];
    HIPCHK(c, hipMemcpy(hdr, c->X.hdr, sizeof(hdr), hipMemcpyDeviceToHost));
    if (hdr[0] < 0 || hdr[0] > c->cap || hdr[1] < 0) return fail(c, PCAMV_EHIP, "extract header corrupt");
    if (n_out) *n_out = hdr[0];
    if (m_out) *m_out = hdr[1];
    const int m_copy = hdr[1] < c->cap ? hdr[1] : c->cap;
    if (bits_out && m_copy) HIPCHK(c, hipMemcpy(bits_out, c->d_rx_bits, (size_t)m_copy, hipMemcpyDeviceToHost));
    return rx_check(c, NULL);
}
/* ------------------------------------------------------------------ slice streams: what the receiver from one and the sender to one share */
/* The stream's entropy mode is stated by the call (cavlc = 0 / 1) and has to be the contexts' (a batch is of one mode): looked at before
 * anything is set up, so that a batch never holds the other mode's tables.
 * for_cavlc / for_cabac: the caller's entry points of either mode and what they do, for the message */
static int entropy_mode(pcamv_batch *b, int cavlc, const char *for_cavlc, const char *for_cabac)
{
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        if (!cavlc && !c->F.b_cabac) return fail(b, PCAMV_EUNSUP, "context %d was opened with --no-cabac: its slices are CAVLC, which %s", i, for_cavlc);
        if (cavlc && c->F.b_cabac) return fail(b, PCAMV_EUNSUP, "context %d was opened with CABAC: its slices are CABAC, which %s", i, for_cabac);
    }
    return 0;
}
/* the tables of a mode as the one block its kernels read, made once: the SV_TAB_BYTES of sv_build_tables, or the standard's CABAC tables
 * init_p[2 * nctx] | transition[256] | range_lps[512] for the nctx contexts the kernel keeps */
static_assert(SP_TAB_INIT == 0 && SP_TAB_TRANS == 2 * SP_NCTX && SP_TAB_RLPS == 2 * SP_NCTX + 256 && SP_TAB_BYTES == 2 * SP_NCTX + 768, "k_parse_pslice reads another table block than entropy_tab makes");
static_assert(SW_TAB_INIT == 0 && SW_TAB_TRANS == 2 * SW_NCTX && SW_TAB_RLPS == 2 * SW_NCTX + 256 && SW_TAB_BYTES == 2 * SW_NCTX + 768, "k_write_pslice reads another table block than entropy_tab makes");
static int entropy_tab(pcamv_batch *b, DevBuf<uint8_t> &d_tab, int cavlc, int nctx)
{
    uint8_t tab[SV_TAB_BYTES > SW_TAB_BYTES ? SV_TAB_BYTES : SW_TAB_BYTES];
    static_assert(SP_NCTX <= SW_NCTX, "entropy_tab's block is sized for the writer's contexts");
    if (d_tab) return 0;
    if (cavlc && sv_build_tables(tab)) return fail(b, PCAMV_EINVAL, "a CAVLC code of pcamv_entropy_tables.h does not fit the %stable entry", &d_tab == &b->d_sp_tab ? "parser's " : "");
    if (!cavlc) { memcpy(tab, pcamv_cabac_init_p, 2 * nctx); memcpy(tab + 2 * nctx, pcamv_cabac_transition, 256); memcpy(tab + 2 * nctx + 256, pcamv_cabac_range_lps, 512); }
    const size_t bytes = cavlc ? (size_t)SV_TAB_BYTES : (size_t)2 * nctx + 768;
    TRY(d_tab.room(b, bytes));
    HIPCHK(b, hipMemcpy(d_tab, tab, bytes, hipMemcpyHostToDevice));
    return 0;
}
/* the row buffers of a launch, one per slice: the bytes of each, and the allocation for pictures too wide for LDS */
static size_t row_bytes(const pcamv_batch *b, int cavlc) { return (size_t)(cavlc ? SV_ROW_BYTES : SP_ROW_BYTES) * b->ctx[0]->F.mb_w; }
/* what every launch of a parser or a writer needs of the batch: status words, the tables of its mode, scratch rows (each made by the
 * first call that needs it, never regrown) */
static int entropy_setup(pcamv_batch *b, DevBuf<int> &d_stat, DevBuf<uint8_t> &d_tab, DevBuf<uint8_t> &d_scratch, int cavlc, int nctx)
{
    if (!d_stat) TRY(d_stat.room(b, (size_t)b->n));
    TRY(entropy_tab(b, d_tab, cavlc, nctx));
    if (b->ctx[0]->F.mb_w > b->sp_lds_cols && !d_scratch) TRY(d_scratch.room(b, (size_t)b->n * row_bytes(b, cavlc)));
    return 0;
}
/* synchronises; the status words of the batch's last parse or write call */
static int status_fetch(pcamv_batch *b, DevBuf<int> pcamv_batch::*d_stat, int32_t *status, const char *none_yet)
{
    if (!b || !status) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    if (!(b->*d_stat)) return fail(b, PCAMV_EINVAL, "%s", none_yet);
    HIPCHK(b, hipDeviceSynchronize());
    HIPCHK(b, hipMemcpy(status, b->*d_stat, sizeof(int32_t) * b->n, hipMemcpyDeviceToHost));
    return 0;
}
/* ------------------------------------------------------------------ receiver from a stream (k_parse_pslice, k_parse_pslice_cavlc, pcamv_slice.hip.h) */
/* the contexts can take parsed slices: (want_rx) a reservation each; their descriptors then point at the receive-side records */
static int slice_contexts(pcamv_batch *b, int want_rx, float emrate)
{
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        if (want_rx && !c->d_rx && !b->d_mrx) return fail(b, PCAMV_EINVAL, "context %d has no received buffer (pcamv_gpu_rx_reserve)", i);
    }
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        TRY(rx_scratch(c)); TRY(rx_mbs(c));
        c->X.mbs = c->d_rx_mbs; c->X.flip = NULL; c->X.bits = NULL; c->X.emrate = emrate; c->X.slice_status = b->d_sstat + i;
        c->win = NULL;
    }
    return 0;
}
/* (a window: `jobs` slices with the window's own scratch rows instead of one per context with the batch's) */
static void slice_launch(pcamv_batch *b, const ExtractDev *dX, SliceJobs J, int cavlc, hipStream_t st, int jobs = 0, uint8_t *scratch = NULL)
{
    const FrameDev &F = b->ctx[0]->F;
    if (!jobs) { jobs = b->n; scratch = b->d_sp_scratch; }
    J.tab = b->d_sp_tab; J.scratch = scratch; J.scratch_stride = (long long)row_bytes(b, cavlc);
    J.mb_w = F.mb_w; J.mb_h = F.mb_h; J.lds_cols = b->sp_lds_cols;
    if (cavlc) timed_kernel(b, KT_PARSE_PSLICE_CAVLC, st, k_parse_pslice_cavlc, dim3(jobs), dim3(64), dX, J);
    else timed_kernel(b, KT_PARSE_PSLICE, st, k_parse_pslice, dim3(jobs), dim3(64), dX, J);
}
/* parse (slices described by J, one per context) and, with extract != 0, the receiver's kernels behind it, all on `st` */
static int slices_run(pcamv_batch *b, SliceJobs J, int cavlc, int extract, float emrate, hipStream_t st, const int *first = NULL)
{
    const ExtractDev *dX; int slot;
    TRY(batch_push_xdescs(b, st, &dX, &slot));
    slice_launch(b, dX, J, cavlc, st);
    if (extract) extract_launch(b, dX, b->n, b->ctx[0]->cap, emrate, st, first);
    TRY(launched(b));
    return ring_release(b, b->xring, slot, st);
}
/* host slices into the next staging buffer: [off n][len n][start_bit n] int64, [qp n] int32 (zeros with cavlc: slice_qp is not read),
 * then the bytes, every slice at a multiple of 4; one copy on `st`.  *stage_out: the buffer's index, to be released (stage_release) once the kernels that read it are queued */
static int slices_stage(pcamv_batch *b, const pcamv_slice_t *sl, int cavlc, hipStream_t st, SliceJobs *J, int *stage_out)
{
    const size_t n = (size_t)b->n, hdr = (n * (3 * 8 + 4) + 15) & ~(size_t)15;
    size_t total = hdr;
    for (size_t i = 0; i < n; i++) {
        if (!sl[i].rbsp || sl[i].len > (size_t)SP_MAX_LEN) return fail(b, PCAMV_EINVAL, "slice %d: no bytes, or more than 2^30 of them", (int)i);
        if (sl[i].start_bit > ((size_t)1 << 40)) return fail(b, PCAMV_EINVAL, "slice %d: start bit %zu is beyond any slice", (int)i, sl[i].start_bit);
        total += (sl[i].len + 3) & ~(size_t)3;
    }
    int k;
    TRY(stage_take(b, b->rx_stage, total, &k));
    uint8_t *h = b->rx_stage.h[k];
    long long *off = (long long *)h, *len = off + n, *start = len + n; int *qp = (int *)(start + n);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = (long long)at; len[i] = (long long)sl[i].len; start[i] = (long long)sl[i].start_bit; qp[i] = cavlc ? 0 : sl[i].slice_qp;
        memcpy(h + hdr + at, sl[i].rbsp, sl[i].len);
        at += (sl[i].len + 3) & ~(size_t)3;
    }
    TRY(stage_send(b, b->rx_stage, k, total, st));
    const uint8_t *d = b->rx_stage.d[k];
    J->bytes = d + hdr; J->bytes_size = (long long)(total - hdr);
    J->off = (const long long *)d; J->len = J->off + n; J->start_bit = J->len + n; J->qp = (const int *)(J->start_bit + n);
    *stage_out = k;
    return 0;
}
static int slices_checked(pcamv_batch *b, float emrate, int want_rx, int cavlc)
{
    if (!b || emrate <= 0) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    TRY(entropy_mode(b, cavlc, "pcamv_gpu_batch_extract_slices_cavlc* and pcamv_gpu_parse_pslice_cavlc_device parse", "pcamv_gpu_batch_extract_slices* and pcamv_gpu_parse_pslice_cabac_device parse"));
    TRY(entropy_setup(b, b->d_sstat, b->d_sp_tab, b->d_sp_scratch, cavlc, SP_NCTX));
    return slice_contexts(b, want_rx, emrate);
}
/* Unescape first (k_nal_to_rbsp, one wavefront per unit, queued on `st`): the n NAL units J describes into the next buffer of nal_stage
 * -- [rbsp_len n] int64, [nal_header n] int32, then J->bytes_size bytes in which unit i's RBSP begins at off[i] -- their return codes into
 * d_status.  J then describes the RBSPs: bytes and len are the library's, off / start_bit / qp stay as they were, and a unit that failed
 * has len -1, which the parsers refuse.  The buffer is taken like a staging buffer: not before the call before the last, whose parser
 * read it, is done.  nal_header (optional): the caller's device array instead of the library's; preload (the probe): host bytes the
 * RBSP buffer holds before the launch.  *stage_out: the buffer, to be released once the kernels that read it are queued */
static int nals_unescape(pcamv_batch *b, int n, SliceJobs *J, int *d_status, int32_t *nal_header, const uint8_t *preload, hipStream_t st, int *stage_out)
{
    const size_t hdr = ((size_t)n * (8 + 4) + 15) & ~(size_t)15;
    int k;
    TRY(stage_take(b, b->nal_stage, hdr + (size_t)J->bytes_size, &k, 0));
    uint8_t *d = b->nal_stage.d[k];
    NalJobs N;
    N.bytes = J->bytes; N.bytes_size = J->bytes_size; N.off = J->off; N.len = J->len;
    N.rbsp_len = (long long *)d; N.nal_header = nal_header ? nal_header : (int *)(N.rbsp_len + n); N.rbsp = d + hdr; N.status = d_status;
    if (preload) HIPCHK(b, hipMemcpyAsync(N.rbsp, preload, (size_t)J->bytes_size, hipMemcpyHostToDevice, st));
    timed_kernel(b, KT_NAL_TO_RBSP, st, k_nal_to_rbsp, dim3(n), dim3(64), N);
    J->bytes = N.rbsp; J->len = N.rbsp_len;
    *stage_out = k;
    return 0;
}
/* what the extract_slices* and extract_nals* calls are: J's slices (nal != 0: NAL units, unescaped first) parsed and sent through the receiver */
static int extract_run(pcamv_batch *b, SliceJobs J, int cavlc, int nal, int32_t *nal_header, float emrate, hipStream_t st)
{
    int kn = -1;
    if (nal) TRY(nals_unescape(b, b->n, &J, b->d_sstat, nal_header, NULL, st, &kn));
    const int rc = slices_run(b, J, cavlc, 1, emrate, st), rc2 = kn >= 0 ? stage_release(b, b->nal_stage, kn, st) : 0;       /* released on every path */
    return rc ? rc : rc2;
}
static int extract_slices_host(pcamv_batch *b, const pcamv_slice_t *slices, int cavlc, int nal, float emrate, void *stream)
{
    if (!slices) return PCAMV_EINVAL;
    TRY(slices_checked(b, emrate, 1, cavlc));
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    SliceJobs J; int k;
    TRY(slices_stage(b, slices, cavlc, st, &J, &k));
    const int rc = extract_run(b, J, cavlc, nal, NULL, emrate, st), rc2 = stage_release(b, b->rx_stage, k, st);      /* released on every path */
    return rc ? rc : rc2;
}
static int extract_slices_device(pcamv_batch *b, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, const int64_t *start_bit,
                                 const int32_t *slice_qp, int cavlc, int nal, int32_t *nal_header, float emrate, void *stream)
{
    if (!bytes || !off || !len || !start_bit || (!cavlc && !slice_qp) || bytes_size > ((size_t)1 << 62)) return PCAMV_EINVAL;
    TRY(slices_checked(b, emrate, 1, cavlc));
    static_assert(sizeof(long long) == sizeof(int64_t), "the caller's int64 arrays are read as they are");
    SliceJobs J;
    J.bytes = (const uint8_t *)bytes; J.bytes_size = (long long)bytes_size;
    J.off = (const long long *)off; J.len = (const long long *)len; J.start_bit = (const long long *)start_bit; J.qp = slice_qp;
    return extract_run(b, J, cavlc, nal, nal_header, emrate, stream ? (hipStream_t)stream : b->ctx[0]->stream);
}
extern "C" int pcamv_gpu_batch_extract_slices(pcamv_batch_t *b, const pcamv_slice_t *slices, float emrate, void *stream)
{
    return extract_slices_host(b, slices, 0, 0, emrate, stream);
}
extern "C" int pcamv_gpu_batch_extract_slices_cavlc(pcamv_batch_t *b, const pcamv_slice_t *slices, float emrate, void *stream)
{
    return extract_slices_host(b, slices, 1, 0, emrate, stream);
}
extern "C" int pcamv_gpu_batch_extract_slices_device(pcamv_batch_t *b, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                                     const int64_t *start_bit, const int32_t *slice_qp, float emrate, void *stream)
{
    if (!slice_qp) return PCAMV_EINVAL;
    return extract_slices_device(b, bytes, bytes_size, off, len, start_bit, slice_qp, 0, 0, NULL, emrate, stream);
}
extern "C" int pcamv_gpu_batch_extract_slices_cavlc_device(pcamv_batch_t *b, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                                           const int64_t *start_bit, float emrate, void *stream)
{
    return extract_slices_device(b, bytes, bytes_size, off, len, start_bit, NULL, 1, 0, NULL, emrate, stream);
}
/* the same four on NAL units */
extern "C" int pcamv_gpu_batch_extract_nals(pcamv_batch_t *b, const pcamv_slice_t *units, float emrate, void *stream)
{
    return extract_slices_host(b, units, 0, 1, emrate, stream);
}
extern "C" int pcamv_gpu_batch_extract_nals_cavlc(pcamv_batch_t *b, const pcamv_slice_t *units, float emrate, void *stream)
{
    return extract_slices_host(b, units, 1, 1, emrate, stream);
}
extern "C" int pcamv_gpu_batch_extract_nals_device(pcamv_batch_t *b, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                                   const int64_t *start_bit, const int32_t *slice_qp, int32_t *nal_header, float emrate, void *stream)
{
    if (!slice_qp) return PCAMV_EINVAL;
    return extract_slices_device(b, bytes, bytes_size, off, len, start_bit, slice_qp, 0, 1, nal_header, emrate, stream);
}
extern "C" int pcamv_gpu_batch_extract_nals_cavlc_device(pcamv_batch_t *b, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                                         const int64_t *start_bit, int32_t *nal_header, float emrate, void *stream)
{
    return extract_slices_device(b, bytes, bytes_size, off, len, start_bit, NULL, 1, 1, nal_header, emrate, stream);
}
/* What the parity probes of the stream kernels open with: the host's (bytes, off[n], len[n]) on the context's device, in temporaries
 * of the probe -- d_at holds `arrays` arrays of n, [off][len] and what the probe keeps behind them */
static int probe_upload(pcamv_ctx *c, DevBuf<uint8_t> &d_bytes, DevBuf<long long> &d_at, const uint8_t *bytes, size_t bytes_size, const int64_t *off,
                        const int64_t *len, int n, int arrays)
{
    HIPCHK(c, hipSetDevice(c->device));
    TRY(d_bytes.room(c, bytes_size ? bytes_size : 1)); TRY(d_at.room(c, (size_t)arrays * (size_t)n));
    if (bytes_size) HIPCHK(c, hipMemcpy(d_bytes, bytes, bytes_size, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_at, off, sizeof(int64_t) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_at + n, len, sizeof(int64_t) * n, hipMemcpyHostToDevice));
    return 0;
}
/* the parity probe of k_nal_to_rbsp: n units of one host buffer through one launch, everything copied back */
extern "C" int pcamv_gpu_nal_to_rbsp_device(pcamv_ctx_t *c, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                            uint8_t *out, int64_t *out_len, int32_t *status, int32_t *nal_header)
{
    if (!c || !bytes || !off || !len || !out || !out_len || !status || n < 0 || bytes_size > ((size_t)1 << 40)) return PCAMV_EINVAL;
    if (!n) return 0;
    pcamv_batch *b = c->self;
    DevBuf<uint8_t> d_bytes; DevBuf<long long> d_at; DevBuf<int> d_status;
    TRY(probe_upload(c, d_bytes, d_at, bytes, bytes_size, off, len, n, 2)); TRY(d_status.room(c, (size_t)n));
    SliceJobs J;
    J.bytes = d_bytes; J.bytes_size = (long long)bytes_size; J.off = d_at; J.len = d_at + n;
    int k;
    TRY(on_behalf(c, b, nals_unescape(b, n, &J, d_status, NULL, out, c->stream, &k)));
    const int rc = launched(b), rc2 = stage_release(b, b->nal_stage, k, c->stream);                  /* released on every path */
    TRY(on_behalf(c, b, rc ? rc : rc2));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, J.bytes, bytes_size, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_len, J.len, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    if (nal_header) HIPCHK(c, hipMemcpy(nal_header, J.len + n, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(status, d_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int pcamv_gpu_batch_slice_status(pcamv_batch_t *b, int32_t *status)
{
    return status_fetch(b, &pcamv_batch::d_sstat, status, "no slices were handed to this batch yet");
}
/* the parity probe: one slice from host bytes through k_parse_pslice (k_parse_pslice_cavlc), its records back */
static int parse_pslice_device(pcamv_ctx_t *c, const uint8_t *rbsp, size_t len, size_t start_bit, int slice_qp, int cavlc, pcamv_mb_t *out_mb)
{
    if (!c || !rbsp || !out_mb) return PCAMV_EINVAL;
    pcamv_batch *b = c->self;
    TRY(on_behalf(c, b, slices_checked(b, 1.0f, 0, cavlc)));
    const pcamv_slice_t sl = {rbsp, len, start_bit, slice_qp};
    SliceJobs J; int k, rc = 0;
    TRY(on_behalf(c, b, slices_stage(b, &sl, cavlc, c->stream, &J, &k)));
    rc = slices_run(b, J, cavlc, 0, 1.0f, c->stream);
    const int rc2 = stage_release(b, b->rx_stage, k, c->stream);                                     /* released on every path */
    TRY(on_behalf(c, b, rc ? rc : rc2));
    rc = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&rc, b->d_sstat, sizeof(rc), hipMemcpyDeviceToHost));
    if (rc) return fail(c, rc, rc == PCAMV_EUNSUP ? "the slice holds an intra macroblock" : cavlc ? "the slice does not parse (a code no table has, bits left over or missing, or a bad start bit)" :
                        "the slice does not parse (ends in the wrong place, runs out of bytes, or bad alignment bits)");
    HIPCHK(c, hipMemcpy(out_mb, c->d_rx_mbs, (size_t)c->F.n_mb * sizeof(pcamv_mb_t), hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int pcamv_gpu_parse_pslice_cabac_device(pcamv_ctx_t *c, const uint8_t *rbsp, size_t len, size_t start_bit, int slice_qp, pcamv_mb_t *out_mb)
{
    return parse_pslice_device(c, rbsp, len, start_bit, slice_qp, 0, out_mb);
}
extern "C" int pcamv_gpu_parse_pslice_cavlc_device(pcamv_ctx_t *c, const uint8_t *rbsp, size_t len, size_t start_bit, pcamv_mb_t *out_mb)
{
    return parse_pslice_device(c, rbsp, len, start_bit, 0, 1, out_mb);
}
/* ------------------------------------------------------------------ receiver on byte streams (k_stream_*, k_slice_header, pcamv_slice.hip.h) */
extern "C" int pcamv_gpu_stream_chunk(void) { return SI_CHUNK; }
/* the device memory of an index of n streams in bytes_size bytes, tables of max_units entries and `guard` more behind each: grown, never
 * shrunk (freeing waits for the device: only a call that may synchronise gets here) */
static int stream_index_room(pcamv_batch *b, StreamIndex &S, int n, long long max_units, int guard, size_t bytes_size)
{
    S.ready = 0;
    S.n = n; S.max_units = max_units; S.stride = max_units + guard;
    S.max_chunks = (long long)(bytes_size / SI_CHUNK) + 2LL * n + 2;
    TRY(S.d_at.room(b, 6 * (size_t)n)); TRY(S.d_bad.room(b, (size_t)n)); TRY(S.d_longest.room(b, 1));
    TRY(S.d_chunks.room(b, (size_t)S.max_chunks));
    return S.d_table.room(b, (size_t)n * (size_t)S.stride);
}
/* the four kernels on `st`: streams (d_off[i], d_len[i]) of d_bytes; all != 0: every unit into the tables, else the slice units */
static int stream_index_run(pcamv_batch *b, StreamIndex &S, const uint8_t *d_bytes, size_t bytes_size, const long long *d_off, const long long *d_len, int all, hipStream_t st)
{
    const size_t n = (size_t)S.n;
    HIPCHK(b, hipMemcpyAsync(S.d_at, d_off, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemcpyAsync(S.d_at + n, d_len, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemsetAsync(S.d_longest, 0, 8, st));
    StreamJobs J;
    J.bytes = d_bytes; J.bytes_size = (long long)bytes_size; J.off = S.d_at; J.len = S.d_at + n;
    J.chunk_base = S.d_at + 2 * n; J.bad = S.d_bad; J.chunks = S.d_chunks; J.max_chunks = S.max_chunks;
    J.table = S.d_table; J.max_units = S.max_units; J.stride = S.stride; J.all = all;
    J.n_units = S.d_at + 3 * n; J.n_slices = S.d_at + 4 * n; J.cursor = S.d_at + 5 * n; J.longest = S.d_longest; J.n = S.n;
    const unsigned chunks = (unsigned)S.max_chunks;
    timed_kernel(b, KT_STREAM_PLAN, st, k_stream_plan, dim3(1), dim3(64), J);
    timed_kernel(b, KT_STREAM_SCAN, st, k_stream_scan<0>, dim3(chunks), dim3(64), J);
    timed_kernel(b, KT_STREAM_PREFIX, st, k_stream_prefix<0>, dim3(S.n), dim3(64), J);
    timed_kernel(b, KT_STREAM_PLACE, st, k_stream_place<0>, dim3(chunks), dim3(64), J);
    return launched(b);
}
static int stream_index_checked(pcamv_batch *b, const void *bytes, size_t bytes_size, long long max_units)
{
    if (!b || !bytes || max_units < 1 || max_units > (1LL << 24) || bytes_size > ((size_t)1 << 40)) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    return batch_live(b);
}
/* the job arrays and RBSP slots of a window of sw.k units per context, sized like a step's for n * k jobs; grown, never shrunk, and only
 * where the device is idle (an index call behind its synchronisation, stream_window) */
static int window_jobs_room(pcamv_batch *b)
{
    StreamWindow &W = b->sw;
    const size_t jobs = (size_t)b->n * (size_t)W.k;
    return W.d_jobs.room(b, stream_step_hdr((int)jobs) + jobs * (size_t)b->sx.slot);
}
/* behind the kernels: the one synchronisation of an index call, the counts to the host, the RBSP slots of the steps to come */
static int stream_index_finish(pcamv_batch *b, const uint8_t *d_bytes, size_t bytes_size, int64_t *n_slices_out)
{
    StreamIndex &S = b->sx;
    HIPCHK(b, hipDeviceSynchronize());
    unsigned long long longest = 0;
    HIPCHK(b, hipMemcpy(&longest, S.d_longest, 8, hipMemcpyDeviceToHost));
    static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as they are");
    if (n_slices_out) HIPCHK(b, hipMemcpy(n_slices_out, S.d_at + 4 * (size_t)S.n, 8 * (size_t)S.n, hipMemcpyDeviceToHost));
    /* an RBSP is shorter than its unit by the header byte at least; slots at multiples of 4 */
    S.slot = (long long)((longest + 3) & ~3ULL); if (S.slot < 4) S.slot = 4;
    const size_t total = stream_step_hdr(S.n) + (size_t)S.n * (size_t)S.slot;
    for (int k = 0; k < NSTAGE; k++) TRY(stage_room(b, b->su_stage, k, total, 0, 0));       /* (every buffer: the steps find their room) */
    S.bytes = d_bytes; S.bytes_size = (long long)bytes_size; S.ready = 1;
    b->ps.ready = 0;                                /* the sets belong to the streams of the index call before */
    b->video = 0;                                   /* (pcamv_gpu_batch_index_video* sets it behind this) */
    return b->sw.k ? window_jobs_room(b) : 0;       /* (a window reserved earlier: its RBSP slots follow, as the steps' do) */
}
extern "C" int pcamv_gpu_batch_index_streams_device(pcamv_batch_t *b, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                                    int64_t max_units, int64_t *n_slices_out, void *stream)
{
    if (!off || !len) return PCAMV_EINVAL;
    TRY(stream_index_checked(b, bytes, bytes_size, max_units));
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    TRY(stream_index_room(b, b->sx, b->n, max_units, 0, bytes_size));
    TRY(stream_index_run(b, b->sx, (const uint8_t *)bytes, bytes_size, (const long long *)off, (const long long *)len, 0, st));
    return stream_index_finish(b, (const uint8_t *)bytes, bytes_size, n_slices_out);
}
/* host streams into a buffer of the index's own -- [off n][len n] int64, then the bytes, every stream at a multiple of 4 -- with one copy */
extern "C" int pcamv_gpu_batch_index_streams(pcamv_batch_t *b, const pcamv_stream_t *streams, int64_t max_units, int64_t *n_slices_out, void *stream)
{
    if (!streams) return PCAMV_EINVAL;
    TRY(stream_index_checked(b, streams, 0, max_units));
    const size_t n = (size_t)b->n, hdr = (16 * n + 15) & ~(size_t)15;
    size_t total = hdr;
    for (size_t i = 0; i < n; i++) {
        if ((!streams[i].bytes && streams[i].len) || streams[i].len > ((size_t)1 << 36)) return fail(b, PCAMV_EINVAL, "stream %d: no bytes, or more than 2^36 of them", (int)i);
        total += (streams[i].len + 3) & ~(size_t)3;
    }
    HostTmp<uint8_t> h(total);
    if (!h) return fail(b, PCAMV_ENOMEM, "no memory to stage %zu bytes of streams", total);
    long long *off = (long long *)h.p, *len = off + n;
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = (long long)at; len[i] = (long long)streams[i].len;
        if (streams[i].len) memcpy(h.p + hdr + at, streams[i].bytes, streams[i].len);
        at += (streams[i].len + 3) & ~(size_t)3;
    }
    StreamIndex &S = b->sx;
    S.ready = 0;
    HIPCHK(b, hipDeviceSynchronize());              /* (steps on the buffer that is replaced may be in flight) */
    TRY(S.d_own.room(b, total));
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    HIPCHK(b, hipMemcpy(S.d_own, h.p, total, hipMemcpyHostToDevice));       /* (complete on return: the host block does not outlive this call) */
    TRY(stream_index_room(b, S, b->n, max_units, 0, total - hdr));
    TRY(stream_index_run(b, S, S.d_own + hdr, total - hdr, (const long long *)S.d_own.p, (const long long *)S.d_own.p + n, 0, st));
    return stream_index_finish(b, S.d_own + hdr, total - hdr, n_slices_out);
}
/* ---- one video (k_video_cut; pcamv_video.h) */
/* The S.n videos (d_off[v], d_len[v]) of d_bytes with ALL their units listed: plan, scan and prefix with a table of no entries give the
 * counts, the one wait for `st` brings them to the host (h_units[S.n]: a video's count, PCAMV_EINVAL for one outside the buffer), the
 * table is made for the largest, and prefix and place run again over the summaries the scan left (kept aside, since the prefix works
 * in place): the bytes are read twice, as by a plain index call */
/* the prefix between scan and place: k_stream_prefix, a wavefront per stream, or for one long stream the same in two levels on many */
template <int SEL> static void video_prefix_launch(pcamv_batch *b, const StreamIndex &S, const StreamJobs &J, hipStream_t st)
{
    timed(b, KT_STREAM_PREFIX, st, [&] {
        if (S.n == 1 && S.d_keep) {
            SiChunk *B = S.d_keep + S.max_chunks;
            const unsigned blocks = (unsigned)((S.max_chunks + VP_BLOCK - 1) / VP_BLOCK);
            hipLaunchKernelGGL(k_video_prefix_local, dim3(blocks), dim3(64), 0, st, J, B);
            hipLaunchKernelGGL(k_video_prefix_top<SEL>, dim3(1), dim3(64), 0, st, J, B);
            hipLaunchKernelGGL(k_video_prefix_apply, dim3((unsigned)((S.max_chunks + 63) / 64)), dim3(64), 0, st, J, B);
        } else hipLaunchKernelGGL(k_stream_prefix<SEL>, dim3(S.n), dim3(64), 0, st, J);
    });
}
static int video_units_run(pcamv_batch *b, StreamIndex &S, const uint8_t *d_bytes, size_t bytes_size, const long long *d_off, const long long *d_len, long long *h_units,
                           hipStream_t st)
{
    const size_t n = (size_t)S.n;
    TRY(stream_index_room(b, S, S.n, 1, 0, bytes_size));
    TRY(S.d_keep.room(b, (size_t)S.max_chunks + (size_t)(S.max_chunks + VP_BLOCK - 1) / VP_BLOCK));    /* (the kept summaries, then the blocks') */
    HIPCHK(b, hipMemcpyAsync(S.d_at, d_off, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemcpyAsync(S.d_at + n, d_len, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemsetAsync(S.d_longest, 0, 8, st));
    StreamJobs J;
    J.bytes = d_bytes; J.bytes_size = (long long)bytes_size; J.off = S.d_at; J.len = S.d_at + n;
    J.chunk_base = S.d_at + 2 * n; J.bad = S.d_bad; J.chunks = S.d_chunks; J.max_chunks = S.max_chunks;
    J.table = S.d_table; J.max_units = 0; J.stride = 0; J.all = 1;
    J.n_units = S.d_at + 3 * n; J.n_slices = S.d_at + 4 * n; J.cursor = S.d_at + 5 * n; J.longest = S.d_longest; J.n = S.n;
    const unsigned chunks = (unsigned)S.max_chunks;
    timed_kernel(b, KT_STREAM_PLAN, st, k_stream_plan, dim3(1), dim3(64), J);
    timed_kernel(b, KT_STREAM_SCAN, st, k_stream_scan<0>, dim3(chunks), dim3(64), J);
    HIPCHK(b, hipMemcpyAsync(S.d_keep, S.d_chunks, (size_t)S.max_chunks * sizeof(SiChunk), hipMemcpyDeviceToDevice, st));
    video_prefix_launch<0>(b, S, J, st);
    TRY(launched(b));
    HIPCHK(b, hipStreamSynchronize(st));
    HIPCHK(b, hipMemcpy(h_units, S.d_at + 3 * n, 8 * n, hipMemcpyDeviceToHost));
    long long most = 1;
    for (size_t v = 0; v < n; v++) if (h_units[v] > most) most = h_units[v];
    if (most > (1LL << 28)) return fail(b, PCAMV_ENOMEM, "a video of %lld units: the table of all of them is limited to 2^28 entries", most);
    S.max_units = most; S.stride = most;
    TRY(S.d_table.room(b, n * (size_t)most));
    J.table = S.d_table; J.max_units = most; J.stride = most;
    HIPCHK(b, hipMemcpyAsync(S.d_chunks, S.d_keep, (size_t)S.max_chunks * sizeof(SiChunk), hipMemcpyDeviceToDevice, st));
    video_prefix_launch<0>(b, S, J, st);
    timed_kernel(b, KT_STREAM_PLACE, st, k_stream_place<0>, dim3(chunks), dim3(64), J);
    return launched(b);
}
static VideoCut video_cut_jobs(const StreamIndex &S)
{
    const size_t n = (size_t)S.n;
    VideoCut Q = VideoCut();
    Q.table = S.d_table; Q.stride = S.stride; Q.n_units = S.d_at + 3 * n; Q.off = S.d_at; Q.len = S.d_at + n; Q.bad = S.d_bad;
    return Q;
}
/* the video (d_off[0], d_len[0]) of d_bytes to the batch's contexts: GOP first_gop + i is context i's stream */
static int index_video_run(pcamv_batch *b, const uint8_t *d_bytes, size_t bytes_size, const long long *d_off, const long long *d_len, long long first_gop,
                           long long max_units, int64_t *n_gops, int64_t *preamble, int64_t *n_slices_out, hipStream_t st)
{
    const size_t n = (size_t)b->n;
    StreamIndex &V = b->vx;
    b->video = 0; b->sx.ready = 0; b->ps.ready = 0;
    /* (the video's own tables and the contexts' (off, len) are read by this call's kernels and by stream_param_sets alone, which waits) */
    TRY(b->d_vcut.room(b, 2 * n + 2));
    V.n = 1;
    long long units = 0;
    TRY(video_units_run(b, V, d_bytes, bytes_size, d_off, d_len, &units, st));
    if (units < 0) return fail(b, PCAMV_EINVAL, "the video does not lie inside the buffer");
    VideoCut Q = video_cut_jobs(V);
    Q.first = first_gop; Q.ctx_off = b->d_vcut; Q.ctx_len = b->d_vcut + n; Q.n_ctx = b->n; Q.n_gops = b->d_vcut + 2 * n; Q.preamble = b->d_vcut + 2 * n + 1;
    timed_kernel(b, KT_VIDEO_CUT, st, k_video_cut, dim3(1), dim3(64), Q);
    TRY(stream_index_room(b, b->sx, b->n, max_units, 0, bytes_size));
    TRY(stream_index_run(b, b->sx, d_bytes, bytes_size, Q.ctx_off, Q.ctx_len, 0, st));
    TRY(stream_index_finish(b, d_bytes, bytes_size, n_slices_out));
    static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as they are");
    if (n_gops) HIPCHK(b, hipMemcpy(n_gops, Q.n_gops, 8, hipMemcpyDeviceToHost));
    if (preamble) HIPCHK(b, hipMemcpy(preamble, Q.preamble, 8, hipMemcpyDeviceToHost));
    b->video = 1;
    return 0;
}
extern "C" int pcamv_gpu_batch_index_video_device(pcamv_batch_t *b, const void *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                                  int64_t first_gop, int64_t max_units, int64_t *n_gops, int64_t *preamble, int64_t *n_slices_out, void *stream)
{
    if (!off || !len || first_gop < 0 || first_gop > (1LL << 40)) return PCAMV_EINVAL;
    TRY(stream_index_checked(b, bytes, bytes_size, max_units));
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    return index_video_run(b, (const uint8_t *)bytes, bytes_size, (const long long *)off, (const long long *)len, first_gop, max_units, n_gops, preamble, n_slices_out, st);
}
/* a host video into the index's own buffer -- [off = 0][len] int64, then the bytes -- with one copy */
extern "C" int pcamv_gpu_batch_index_video(pcamv_batch_t *b, const uint8_t *bytes, size_t len, int64_t first_gop, int64_t max_units, int64_t *n_gops,
                                           int64_t *preamble, int64_t *n_slices_out, void *stream)
{
    if ((!bytes && len) || len > ((size_t)1 << 36) || first_gop < 0 || first_gop > (1LL << 40)) return PCAMV_EINVAL;
    TRY(stream_index_checked(b, b, 0, max_units));
    StreamIndex &S = b->sx;
    S.ready = 0;
    HIPCHK(b, hipDeviceSynchronize());              /* (steps on the buffer that is replaced may be in flight) */
    TRY(S.d_own.room(b, 16 + len));
    const long long at[2] = {0, (long long)len};
    HIPCHK(b, hipMemcpy(S.d_own, at, 16, hipMemcpyHostToDevice));
    if (len) HIPCHK(b, hipMemcpy(S.d_own + 16, bytes, len, hipMemcpyHostToDevice));
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    return index_video_run(b, S.d_own + 16, len, (const long long *)S.d_own.p, (const long long *)S.d_own.p + 1, first_gop, max_units, n_gops, preamble, n_slices_out, st);
}
/* the parity probe of the cut: n videos of one host buffer, every video's units listed and walked by a wavefront of its own */
extern "C" int pcamv_gpu_video_gops_device(pcamv_ctx_t *c, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                           pcamv_gop_t *gops_out, int64_t cap_per_video, int64_t *n_gops, int64_t *preamble)
{
    if (!c || (!bytes && bytes_size) || !off || !len || !gops_out || !n_gops || !preamble || n < 1 || n > (1 << 20) || cap_per_video < 0 ||
        cap_per_video > (1LL << 24) || bytes_size > ((size_t)1 << 40)) return PCAMV_EINVAL;
    pcamv_batch *b = c->self;
    const size_t entries = (size_t)n * (size_t)(cap_per_video + PCAMV_UNIT_GUARD);
    DevBuf<uint8_t> d_bytes; DevBuf<long long> d_at; DevBuf<pcamv_gop_t> d_gops;
    TRY(probe_upload(c, d_bytes, d_at, bytes, bytes_size, off, len, n, 4)); TRY(d_gops.room(c, entries));
    HIPCHK(c, hipMemset(d_gops, 0xA5, entries * sizeof(pcamv_gop_t)));
    HostTmp<long long> h_units((size_t)n);
    if (!h_units) return fail(c, PCAMV_ENOMEM, "no memory for the counts of %d videos", n);
    StreamIndex S{};            /* (the probe's own index: freed with the scope) */
    S.n = n;
    TRY(on_behalf(c, b, video_units_run(b, S, d_bytes, bytes_size, d_at, d_at + n, h_units, c->stream)));
    VideoCut Q = video_cut_jobs(S);
    Q.gops = d_gops; Q.gstride = cap_per_video + PCAMV_UNIT_GUARD; Q.cap = cap_per_video;
    Q.n_gops = d_at + 2 * (size_t)n; Q.preamble = d_at + 3 * (size_t)n;
    timed_kernel(b, KT_VIDEO_CUT, c->stream, k_video_cut, dim3(n), dim3(64), Q);
    TRY(on_behalf(c, b, launched(b)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(gops_out, d_gops, entries * sizeof(pcamv_gop_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(n_gops, d_at + 2 * (size_t)n, 8 * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(preamble, d_at + 3 * (size_t)n, 8 * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}
/* the entropy mode of a *_sets call is the contexts' own: 1 CAVLC, 0 CABAC (a batch holds contexts of one mode: pcamv_gpu_batch_create) */
static int sets_mode(pcamv_batch *b, int *cavlc)
{
    if (!b) return PCAMV_EINVAL;
    TRY(batch_live(b));
    *cavlc = !b->ctx[0]->F.b_cabac;
    return 0;
}
/* the header stage of a step or a window: under `params`, or (NULL) under every context's own sets */
static void slice_header_launch(pcamv_batch *b, StreamStep &J, const pcamv_stream_params_t *params, int cavlc, int sets_k, size_t jobs, hipStream_t st)
{
    J.sets = NULL; J.sets_k = sets_k; J.want_cabac = !cavlc; J.entropy = J.frame_num + 2 * jobs;
    if (params) {
        J.P = *params;
        timed_kernel(b, KT_SLICE_HEADER, st, k_slice_header, dim3((unsigned)((jobs + 63) / 64)), dim3(64), J);
    } else {
        J.P = pcamv_stream_params_t();
        J.sets = b->ps.d_sets;
        timed_kernel(b, KT_SLICE_HEADER_SETS, st, k_slice_header_sets, dim3((unsigned)((jobs + 63) / 64)), dim3(64), J);
    }
}
static int extract_stream_step(pcamv_batch_t *b, const pcamv_stream_params_t *params, float emrate, int32_t *nal_header, void *stream)
{
    int cavlc = 0;
    if (params) cavlc = !params->entropy_cabac; else TRY(sets_mode(b, &cavlc));
    TRY(slices_checked(b, emrate, 1, cavlc));
    StreamIndex &S = b->sx;
    if (!S.ready) return fail(b, PCAMV_EINVAL, "no byte streams were handed to this batch yet (pcamv_gpu_batch_index_streams*)");
    if (!params && !b->ps.ready) return fail(b, PCAMV_EINVAL, "the parameter sets of the indexed streams were not read yet (pcamv_gpu_batch_stream_param_sets behind the index call)");
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    const size_t n = (size_t)b->n, hdr = stream_step_hdr(b->n);
    int k;
    TRY(stage_take(b, b->su_stage, hdr + n * (size_t)S.slot, &k, 0));     /* (never regrown here: the index call sized every buffer) */
    uint8_t *d = b->su_stage.d[k];
    StreamStep J;
    J.bytes = S.bytes; J.bytes_size = S.bytes_size; J.soff = S.d_at; J.slen = S.d_at + n; J.bad = S.d_bad;
    J.table = S.d_table; J.max_units = S.max_units; J.stride = S.stride; J.n_slices = S.d_at + 4 * n; J.cursor = S.d_at + 5 * n;
    J.rbsp = d + hdr; J.slot = S.slot; J.rbsp_size = (long long)n * S.slot;
    J.off = (long long *)d; J.len = J.off + n; J.start_bit = J.len + n;
    J.qp = (int *)(J.start_bit + n); J.first = J.qp + n; J.frame_num = J.first + n; J.nal_header = nal_header ? nal_header : J.frame_num + n;
    J.n = b->n; J.cursor_was = NULL; J.k = 0;
    timed_kernel(b, KT_STREAM_UNIT, st, k_stream_unit, dim3(b->n), dim3(64), J);
    slice_header_launch(b, J, params, cavlc, 1, n, st);
    SliceJobs SJ;
    SJ.bytes = J.rbsp; SJ.bytes_size = J.rbsp_size; SJ.off = J.off; SJ.len = J.len; SJ.start_bit = J.start_bit; SJ.qp = cavlc ? NULL : J.qp;
    const int rc = slices_run(b, SJ, cavlc, 1, emrate, st, J.first);
    /* the parser refused what an earlier stage had failed (len -1) with its own code: the first stage's code takes its place */
    timed_kernel(b, KT_STREAM_STATUS, st, k_stream_status, dim3((b->n + 63) / 64), dim3(64), J.first, b->d_sstat, b->n, (int *)NULL, 0);
    const int rc1 = launched(b), rc2 = stage_release(b, b->su_stage, k, st);        /* released on every path */
    return rc ? rc : rc1 ? rc1 : rc2;
}
extern "C" int pcamv_gpu_batch_extract_stream_step(pcamv_batch_t *b, const pcamv_stream_params_t *params, float emrate, int32_t *nal_header, void *stream)
{
    if (!b || !params) return PCAMV_EINVAL;
    return extract_stream_step(b, params, emrate, nal_header, stream);
}
extern "C" int pcamv_gpu_batch_extract_stream_step_sets(pcamv_batch_t *b, float emrate, int32_t *nal_header, void *stream)
{
    if (!b) return PCAMV_EINVAL;
    return extract_stream_step(b, NULL, emrate, nal_header, stream);
}
/* ---- a window of slice units per context in one launch (k_stream_window_unit, k_extract_count, k_extract_chain) */
/* the window as a new batch has it: what it owned is freed (which waits for the device), every field is zero again.  Destroyed and
 * value-initialised in place, so that no list of its members stands here: they are buffers, a ring and plain data, whose making cannot fail */
static void window_release(StreamWindow &W) { W.~StreamWindow(); new (&W) StreamWindow(); }
/* the memory of a window of k on a released one, for pcamv_gpu_batch_stream_window (below); a failure leaves the clean-up to it */
static int window_reserve(pcamv_batch *b, int k)
{
    StreamWindow &W = b->sw;
    if (!b->sx.ready) return fail(b, PCAMV_EINVAL, "no byte streams were handed to this batch yet (pcamv_gpu_batch_index_streams*): a window is reserved behind an index call");
    const FrameDev &F = b->ctx[0]->F;
    const int cavlc = !F.b_cabac, cap = b->ctx[0]->cap;
    TRY(entropy_setup(b, b->d_sstat, b->d_sp_tab, b->d_sp_scratch, cavlc, SP_NCTX));
    for (int i = 0; i < b->n; i++) {            /* what the first slice call of a context makes: here, so that the window call finds it */
        pcamv_ctx *c = b->ctx[i];
        int rc_c = rx_scratch(c);
        if (!rc_c) rc_c = rx_mbs(c);
        if (rc_c) return fail(b, rc_c, "context %d: %s", i, c->err);
    }
    const size_t jobs = (size_t)b->n * (size_t)k, rec = (size_t)F.n_mb + SLICE_GUARD_MBS;
    W.k = k;
    /* (a device without the memory for the window is PCAMV_ENOMEM here: the caller can reserve a smaller one) */
    TRY(W.d_mbs.room(b, jobs * rec, PCAMV_ENOMEM)); TRY(W.d_stego.room(b, jobs * (size_t)cap, PCAMV_ENOMEM));
    TRY(W.d_hdr.room(b, jobs * 8, PCAMV_ENOMEM)); TRY(W.d_cols.room(b, jobs * 2 * STC_MAXW, PCAMV_ENOMEM)); TRY(W.d_stat.room(b, jobs, PCAMV_ENOMEM));
    if (F.mb_w > b->sp_lds_cols) TRY(W.d_scratch.room(b, jobs * row_bytes(b, cavlc), PCAMV_ENOMEM));
    TRY(W.d_cursor_was.room(b, (size_t)b->n, PCAMV_ENOMEM));
    TRY(W.d_X.room(b, jobs * NSTAGE, PCAMV_ENOMEM)); TRY(W.h_X.room(b, jobs * NSTAGE, PCAMV_ENOMEM));
    HIPCHK(b, hipEventCreateWithFlags(&W.done, hipEventDisableTiming));
    HIPCHK(b, hipMemset(W.d_hdr, 0, jobs * 8 * sizeof(int)));
    HIPCHK(b, hipMemset(W.d_stat, 0, jobs * sizeof(int)));
    /* the guard behind every slot's records, as rx_mbs leaves it behind a context's */
    HIPCHK(b, hipMemset2D(W.d_mbs + F.n_mb, rec * sizeof(pcamv_mb_t), 0xA5, SLICE_GUARD_MBS * sizeof(pcamv_mb_t), jobs));
    return window_jobs_room(b);
}
extern "C" int pcamv_gpu_batch_stream_window(pcamv_batch_t *b, int k)
{
    if (!b || k < 0 || k > PCAMV_STREAM_WINDOW_MAX) return fail(b, PCAMV_EINVAL, "a window holds 1 to %d units per context (0 releases it)", PCAMV_STREAM_WINDOW_MAX);
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    HIPCHK(b, hipDeviceSynchronize());
    window_release(b->sw);
    for (int i = 0; i < b->n; i++) if (b->ctx[i]->win == b) b->ctx[i]->win = NULL;
    if (!k) return 0;
    const int rc = window_reserve(b, k);
    if (rc) window_release(b->sw);
    return rc;
}
static int extract_stream_window(pcamv_batch_t *b, const pcamv_stream_params_t *params, float emrate, int k, int32_t *nal_header, void *stream)
{
    int cavlc = 0;
    if (params) cavlc = !params->entropy_cabac; else TRY(sets_mode(b, &cavlc));
    TRY(slices_checked(b, emrate, 1, cavlc));
    StreamIndex &S = b->sx;
    StreamWindow &W = b->sw;
    if (!S.ready) return fail(b, PCAMV_EINVAL, "no byte streams were handed to this batch yet (pcamv_gpu_batch_index_streams*)");
    if (!params && !b->ps.ready) return fail(b, PCAMV_EINVAL, "the parameter sets of the indexed streams were not read yet (pcamv_gpu_batch_stream_param_sets behind the index call)");
    if (!W.k) return fail(b, PCAMV_EINVAL, "no window was reserved for this batch (pcamv_gpu_batch_stream_window)");
    if (k < 1 || k > W.k) return fail(b, PCAMV_EINVAL, "a window of %d units: 1 to the %d reserved", k, W.k);
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    const FrameDev &F = b->ctx[0]->F;
    const size_t n = (size_t)b->n, jobs = n * (size_t)k, hdr = stream_step_hdr((int)jobs), rec = (size_t)F.n_mb + SLICE_GUARD_MBS;
    const int cap = b->ctx[0]->cap;
    if (hdr + jobs * (size_t)S.slot > W.d_jobs.cap) return fail(b, PCAMV_EHIP, "the window's RBSP slots were not sized by the last index call");
    if (W.used) HIPCHK(b, hipStreamWaitEvent(st, W.done, 0));           /* the call before this one read and wrote the same slots, perhaps on another stream: before anything is written */
    int r;
    TRY(ring_take(b, W.desc, &r));                                      /* (as a step's descriptor ring: the call before the last) */
    ExtractDev *hX = W.h_X + (size_t)r * n * (size_t)W.k, *dX = W.d_X + (size_t)r * n * (size_t)W.k;
    for (size_t i = 0; i < n; i++)
        for (size_t w = 0; w < (size_t)k; w++) {
            const size_t j = i * (size_t)k + w;
            ExtractDev &X = hX[j];
            X = b->ctx[i]->X;
            X.mbs = W.d_mbs + j * rec; X.stego = W.d_stego + j * (size_t)cap; X.hdr = W.d_hdr + j * 8; X.cols = W.d_cols + j * 2 * STC_MAXW;
            X.slice_status = W.d_stat + j;
            if (b->d_mrx) { X.rx = b->d_mrx; X.rx_cap_bits = b->mrx_bits; }
        }
    HIPCHK(b, hipMemcpyAsync(dX, hX, sizeof(ExtractDev) * jobs, hipMemcpyHostToDevice, st));
    /* (the slot's event is recorded once, by ring_release behind the last kernel, and not here behind the copy as well, as stage_send does
     * for a staging buffer: only the copy below can return in between, and only with an error of the runtime, which the call reports) */
    HIPCHK(b, hipMemcpyAsync(W.d_cursor_was, S.d_at + 5 * n, 8 * n, hipMemcpyDeviceToDevice, st));
    uint8_t *d = W.d_jobs;
    StreamStep J;
    J.bytes = S.bytes; J.bytes_size = S.bytes_size; J.soff = S.d_at; J.slen = S.d_at + n; J.bad = S.d_bad;
    J.table = S.d_table; J.max_units = S.max_units; J.stride = S.stride; J.n_slices = S.d_at + 4 * n; J.cursor = S.d_at + 5 * n;
    J.rbsp = d + hdr; J.slot = S.slot; J.rbsp_size = (long long)jobs * S.slot;
    J.off = (long long *)d; J.len = J.off + jobs; J.start_bit = J.len + jobs;
    J.qp = (int *)(J.start_bit + jobs); J.first = J.qp + jobs; J.frame_num = J.first + jobs; J.nal_header = nal_header ? nal_header : J.frame_num + jobs;
    J.n = (int)jobs; J.cursor_was = W.d_cursor_was; J.k = k;
    timed_kernel(b, KT_STREAM_WINDOW_UNIT, st, k_stream_window_unit, dim3((unsigned)jobs), dim3(64), J);
    slice_header_launch(b, J, params, cavlc, k, jobs, st);
    SliceJobs SJ;
    SJ.bytes = J.rbsp; SJ.bytes_size = J.rbsp_size; SJ.off = J.off; SJ.len = J.len; SJ.start_bit = J.start_bit; SJ.qp = cavlc ? NULL : J.qp;
    slice_launch(b, dX, SJ, cavlc, st, (int)jobs, W.d_scratch);
    timed_kernel(b, KT_EXTRACT_COUNT, st, k_extract_count, dim3((unsigned)jobs), dim3(1024), dX);
    if (b->d_mrx) extract_message_chain_launch(b, dX, k, J.first, st);
    else timed_kernel(b, KT_EXTRACT_CHAIN, st, k_extract_chain, dim3((b->n + 63) / 64), dim3(64), dX, b->n, k);
    extract_bits_launch(b, dX, (int)jobs, cap, emrate, st);
    timed_kernel(b, KT_STREAM_STATUS, st, k_stream_status, dim3((unsigned)((jobs + 63) / 64)), dim3(64), J.first, W.d_stat, (int)jobs, b->d_sstat, k);
    W.k_last = k;
    for (int i = 0; i < b->n; i++) { b->ctx[i]->win = b; b->ctx[i]->win_i = i; }
    const int rc = launched(b);
    TRY(ring_release(b, W.desc, r, st));                    /* the descriptors are read until here: behind the last kernel that reads them */
    HIPCHK(b, hipEventRecord(W.done, st));
    W.used = 1;
    return rc;
}
extern "C" int pcamv_gpu_batch_extract_stream_window(pcamv_batch_t *b, const pcamv_stream_params_t *params, float emrate, int k, int32_t *nal_header, void *stream)
{
    if (!b || !params) return PCAMV_EINVAL;
    return extract_stream_window(b, params, emrate, k, nal_header, stream);
}
extern "C" int pcamv_gpu_batch_extract_stream_window_sets(pcamv_batch_t *b, float emrate, int k, int32_t *nal_header, void *stream)
{
    if (!b) return PCAMV_EINVAL;
    return extract_stream_window(b, NULL, emrate, k, nal_header, stream);
}
extern "C" int pcamv_gpu_batch_window_status(pcamv_batch_t *b, int32_t *status)
{
    if (!b || !status) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    if (!b->sw.k || !b->sw.k_last) return fail(b, PCAMV_EINVAL, "no window call was made on this batch yet");
    HIPCHK(b, hipDeviceSynchronize());
    HIPCHK(b, hipMemcpy(status, b->sw.d_stat, sizeof(int32_t) * (size_t)b->n * (size_t)b->sw.k_last, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int pcamv_gpu_batch_stream_tell(pcamv_batch_t *b, int64_t *next, int64_t *total)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    const StreamIndex &S = b->sx;
    if (!S.ready) return fail(b, PCAMV_EINVAL, "no byte streams were handed to this batch yet (pcamv_gpu_batch_index_streams*)");
    HIPCHK(b, hipDeviceSynchronize());
    if (total) HIPCHK(b, hipMemcpy(total, S.d_at + 4 * (size_t)S.n, 8 * (size_t)S.n, hipMemcpyDeviceToHost));
    if (next) HIPCHK(b, hipMemcpy(next, S.d_at + 5 * (size_t)S.n, 8 * (size_t)S.n, hipMemcpyDeviceToHost));
    return 0;
}
/* the parity probe of the index kernels: n streams of one host buffer, all units listed, tables and guards back as the device left them */
extern "C" int pcamv_gpu_index_streams_probe(pcamv_ctx_t *c, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                             pcamv_unit_t *units_out, int64_t cap_per_stream, int64_t *n_units, int64_t *n_slices)
{
    if (!c || (!bytes && bytes_size) || !off || !len || !units_out || !n_units || !n_slices || n < 1 || cap_per_stream < 0 || cap_per_stream > (1LL << 24) ||
        bytes_size > ((size_t)1 << 40)) return PCAMV_EINVAL;
    pcamv_batch *b = c->self;
    DevBuf<uint8_t> d_bytes; DevBuf<long long> d_at;
    TRY(probe_upload(c, d_bytes, d_at, bytes, bytes_size, off, len, n, 2));
    StreamIndex S{};            /* (the probe's own index: freed with the scope) */
    TRY(on_behalf(c, b, stream_index_room(b, S, n, cap_per_stream, PCAMV_UNIT_GUARD, bytes_size)));
    const size_t entries = (size_t)n * (size_t)(cap_per_stream + PCAMV_UNIT_GUARD);
    HIPCHK(c, hipMemsetAsync(S.d_table, 0xA5, entries * sizeof(pcamv_unit_t), c->stream));      /* (guards included: they come back as they were left) */
    TRY(on_behalf(c, b, stream_index_run(b, S, d_bytes, bytes_size, d_at, d_at + n, 1, c->stream)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(units_out, S.d_table, entries * sizeof(pcamv_unit_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(n_units, S.d_at + 3 * (size_t)n, 8 * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(n_slices, S.d_at + 4 * (size_t)n, 8 * (size_t)n, hipMemcpyDeviceToHost));
    HostTmp<uint8_t> back(bytes_size ? bytes_size : 1);
    if (back && bytes_size) {
        HIPCHK(c, hipMemcpy(back.p, d_bytes, bytes_size, hipMemcpyDeviceToHost));
        if (memcmp(back.p, bytes, bytes_size)) return fail(c, PCAMV_EHIP, "the index kernels changed the streams' bytes");
    }
    return 0;
}
/* the parity probe of k_slice_header: n RBSPs of one host buffer, one lane each */
extern "C" int pcamv_gpu_slice_headers_device(pcamv_ctx_t *c, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len,
                                              const int32_t *nal_header, int n, const pcamv_stream_params_t *params, int32_t *rc_out, int64_t *start_bit,
                                              int32_t *slice_qp, int32_t *frame_num)
{
    if (!c || (!bytes && bytes_size) || !off || !len || !nal_header || !params || !rc_out || !start_bit || !slice_qp || !frame_num || n < 1 ||
        bytes_size > ((size_t)1 << 40)) return PCAMV_EINVAL;
    pcamv_batch *b = c->self;
    DevBuf<uint8_t> d_bytes; DevBuf<long long> d_at; DevBuf<int> d_int;
    TRY(probe_upload(c, d_bytes, d_at, bytes, bytes_size, off, len, n, 3)); TRY(d_int.room(c, 4 * (size_t)n));
    HIPCHK(c, hipMemset(d_int, 0, sizeof(int) * 4 * (size_t)n));
    HIPCHK(c, hipMemcpy(d_int + 2 * (size_t)n, nal_header, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    StreamStep J = StreamStep();
    J.rbsp = d_bytes; J.rbsp_size = (long long)bytes_size; J.off = d_at; J.len = d_at + n; J.start_bit = d_at + 2 * (size_t)n;
    J.qp = d_int; J.first = d_int + n; J.nal_header = d_int + 2 * (size_t)n; J.frame_num = d_int + 3 * (size_t)n;
    J.P = *params; J.n = n;
    timed_kernel(b, KT_SLICE_HEADER, c->stream, k_slice_header, dim3((n + 63) / 64), dim3(64), J);
    TRY(on_behalf(c, b, launched(b)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(start_bit, J.start_bit, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(slice_qp, J.qp, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(rc_out, J.first, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(frame_num, J.frame_num, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}
/* ---- parameter sets per stream (k_pset_unit, k_pset_parse, k_pset_resolve; pcamv_param_sets.h) */
/* The streams S indexed (placement, chunk bases and refusals are S's; its chunk summaries are working memory again) through the scan
 * that selects units of type 7 / 8 and the three kernels, on `st`.  Waits for `st` twice: for the counts, by which the per-unit memory is
 * sized (the map of the units goes up with blocking copies), and at the end.  want_w / want_h: the picture size every stream must have, 0: any */
static int pset_run(pcamv_batch *b, const StreamIndex &S, const uint8_t *d_bytes, long long bytes_size, StreamSets &P, int want_w, int want_h, hipStream_t st)
{
    const size_t n = (size_t)S.n;
    P.ready = 0;
    TRY(P.d_table.room(b, n * PCAMV_PSET_UNITS_MAX)); TRY(P.d_cnt.room(b, 3 * n + 1)); TRY(P.d_sets.room(b, n));
    HIPCHK(b, hipMemsetAsync(P.d_cnt, 0, 8 * (3 * n + 1), st));
    StreamJobs J;
    J.bytes = d_bytes; J.bytes_size = bytes_size; J.off = S.d_at; J.len = S.d_at + n;
    J.chunk_base = S.d_at + 2 * n; J.bad = S.d_bad; J.chunks = S.d_chunks; J.max_chunks = S.max_chunks;
    J.table = P.d_table; J.max_units = PCAMV_PSET_UNITS_MAX; J.stride = PCAMV_PSET_UNITS_MAX; J.all = 0;
    J.n_units = P.d_cnt; J.n_slices = P.d_cnt + n; J.cursor = NULL; J.longest = NULL; J.n = S.n;
    const unsigned chunks = (unsigned)S.max_chunks;
    timed_kernel(b, KT_STREAM_SCAN, st, k_stream_scan<SI_SEL_PSET>, dim3(chunks), dim3(64), J);
    video_prefix_launch<SI_SEL_PSET>(b, S, J, st);          /* (k_stream_prefix, but for a video's own index: one long stream) */
    timed_kernel(b, KT_STREAM_PLACE, st, k_stream_place<SI_SEL_PSET>, dim3(chunks), dim3(64), J);
    TRY(launched(b));
    HIPCHK(b, hipStreamSynchronize(st));
    /* the launch's units, stream by stream: the first PCAMV_PSET_UNITS_MAX of each stream the index took */
    HostTmp<long long> h_cnt(2 * n + 1); HostTmp<int> h_bad(n ? n : 1);
    if (!h_cnt || !h_bad) return fail(b, PCAMV_ENOMEM, "no memory for the counts of %zu streams", n);
    HIPCHK(b, hipMemcpy(h_cnt, P.d_cnt + n, 8 * n, hipMemcpyDeviceToHost));
    HIPCHK(b, hipMemcpy(h_bad, S.d_bad, 4 * n, hipMemcpyDeviceToHost));
    long long *h_base = h_cnt + n;
    size_t units = 0;
    for (size_t i = 0; i < n; i++) {
        const long long c = h_bad[i] || h_cnt[i] < 0 ? 0 : h_cnt[i] < PCAMV_PSET_UNITS_MAX ? h_cnt[i] : PCAMV_PSET_UNITS_MAX;
        h_base[i] = (long long)units;
        units += (size_t)c;
    }
    h_base[n] = (long long)units;
    const size_t U = units ? units : 1;
    HostTmp<int> h_map(2 * U);
    if (!h_map) return fail(b, PCAMV_ENOMEM, "no memory for the places of %zu parameter-set units", units);
    for (size_t i = 0; i < n; i++)
        for (long long x = 0; x < h_base[i + 1] - h_base[i]; x++) { h_map[h_base[i] + x] = (int)i; h_map[U + h_base[i] + x] = (int)x; }
    TRY(P.d_len.room(b, U)); TRY(P.d_map.room(b, 4 * U)); TRY(P.d_rec.room(b, U)); TRY(P.d_slots.room(b, U * PCAMV_PSET_UNIT_BYTES));
    HIPCHK(b, hipMemcpy(P.d_map, h_map, 4 * 2 * U, hipMemcpyHostToDevice));
    HIPCHK(b, hipMemcpy(P.d_cnt + 2 * n, h_base, 8 * (n + 1), hipMemcpyHostToDevice));
    PsetJobs Q;
    Q.bytes = d_bytes; Q.bytes_size = bytes_size; Q.soff = S.d_at; Q.slen = S.d_at + n; Q.bad = S.d_bad;
    Q.table = P.d_table; Q.count = P.d_cnt + n;
    Q.u_stream = P.d_map; Q.u_index = P.d_map + U; Q.u_base = P.d_cnt + 2 * n; Q.n_units = (int)units;
    Q.slots = P.d_slots; Q.rbsp_len = P.d_len; Q.nal_header = P.d_map + 2 * U; Q.first = P.d_map + 3 * U; Q.rec = P.d_rec;
    Q.sets = P.d_sets; Q.n = S.n; Q.want_w = want_w; Q.want_h = want_h;
    if (units) {
        timed_kernel(b, KT_PSET_UNIT, st, k_pset_unit, dim3((unsigned)units), dim3(64), Q);
        timed_kernel(b, KT_PSET_PARSE, st, k_pset_parse, dim3((unsigned)((units + 63) / 64)), dim3(64), Q);
    }
    timed_kernel(b, KT_PSET_RESOLVE, st, k_pset_resolve, dim3(S.n), dim3(64), Q);
    TRY(launched(b));
    HIPCHK(b, hipStreamSynchronize(st));
    return 0;
}
extern "C" int pcamv_gpu_batch_stream_param_sets(pcamv_batch_t *b, int32_t *status_out, pcamv_param_sets_t *sets_out, void *stream)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    const StreamIndex &S = b->sx;
    if (!S.ready) return fail(b, PCAMV_EINVAL, "no byte streams were handed to this batch yet (pcamv_gpu_batch_index_streams*)");
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    HIPCHK(b, hipDeviceSynchronize());              /* (steps under the sets that are replaced may be in flight) */
    const size_t n = (size_t)S.n;
    if (b->video) {         /* the video's sets, resolved once, are every context's: GOPs behind the first often carry none of their own */
        TRY(pset_run(b, b->vx, S.bytes, S.bytes_size, b->vps, b->ctx[0]->F.mb_w, b->ctx[0]->F.mb_h, st));
        TRY(b->ps.d_sets.room(b, n));
        hipLaunchKernelGGL(k_pset_spread, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, b->vps.d_sets.p, b->ps.d_sets.p, (int)n);
        TRY(launched(b));
        HIPCHK(b, hipStreamSynchronize(st));
    } else TRY(pset_run(b, S, S.bytes, S.bytes_size, b->ps, b->ctx[0]->F.mb_w, b->ctx[0]->F.mb_h, st));
    if (status_out || sets_out) {
        HostTmp<pcamv_param_sets_t> h(n);
        if (!h) return fail(b, PCAMV_ENOMEM, "no memory for the sets of %zu streams", n);
        HIPCHK(b, hipMemcpy(h, b->ps.d_sets, n * sizeof(pcamv_param_sets_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n && status_out; i++) status_out[i] = h[i].status;
        if (sets_out) memcpy(sets_out, h, n * sizeof(pcamv_param_sets_t));
    }
    b->ps.ready = 1;
    return 0;
}
/* the parity probe: n streams of one host buffer through the index kernels (for their chunks) and the parameter-set kernels */
extern "C" int pcamv_gpu_param_sets_device(pcamv_ctx_t *c, const uint8_t *bytes, size_t bytes_size, const int64_t *off, const int64_t *len, int n,
                                           pcamv_param_sets_t *sets_out)
{
    if (!c || (!bytes && bytes_size) || !off || !len || !sets_out || n < 1 || bytes_size > ((size_t)1 << 40)) return PCAMV_EINVAL;
    pcamv_batch *b = c->self;
    DevBuf<uint8_t> d_bytes; DevBuf<long long> d_at;
    TRY(probe_upload(c, d_bytes, d_at, bytes, bytes_size, off, len, n, 2));
    StreamIndex S{}; StreamSets P{};    /* (the probe's own: freed with the scope) */
    TRY(on_behalf(c, b, stream_index_room(b, S, n, 1, 0, bytes_size)));
    TRY(on_behalf(c, b, stream_index_run(b, S, d_bytes, bytes_size, d_at, d_at + n, 0, c->stream)));
    TRY(on_behalf(c, b, pset_run(b, S, d_bytes, (long long)bytes_size, P, 0, 0, c->stream)));
    HIPCHK(c, hipMemcpy(sets_out, P.d_sets, (size_t)n * sizeof(pcamv_param_sets_t), hipMemcpyDeviceToHost));
    return 0;
}
/* the inverse, host code: what the parsers read, written (pcamv_param_sets.h) */
extern "C" int pcamv_gpu_write_sps(const pcamv_sps_t *sps, uint8_t *rbsp, size_t cap, size_t *len)
{
    if (len) *len = 0;
    if (!sps || !len || (!rbsp && cap)) return PCAMV_EINVAL;
    uint8_t tmp[PCAMV_PSET_RBSP_MAX];
    const int n = ps_write_sps(*sps, tmp);
    if (n < 0) return n;
    if ((size_t)n > cap) return PCAMV_ENOMEM;
    memcpy(rbsp, tmp, (size_t)n);
    *len = (size_t)n;
    return 0;
}
extern "C" int pcamv_gpu_write_pps(const pcamv_pps_t *pps, uint8_t *rbsp, size_t cap, size_t *len)
{
    if (len) *len = 0;
    if (!pps || !len || (!rbsp && cap)) return PCAMV_EINVAL;
    uint8_t tmp[PCAMV_PSET_RBSP_MAX];
    const int n = ps_write_pps(*pps, tmp);
    if (n < 0) return n;
    if ((size_t)n > cap) return PCAMV_ENOMEM;
    memcpy(rbsp, tmp, (size_t)n);
    *len = (size_t)n;
    return 0;
}
extern "C" int pcamv_gpu_rbsp_to_nal(const uint8_t *rbsp, size_t len, int nal_ref_idc, int nal_unit_type, uint8_t *nal, size_t cap, size_t *nal_len);
/* crop_right / crop_bottom: luma samples of the coded picture that are not the picture's, both even */
static int param_set_head_at(const pcamv_stream_params_t *params, int mb_w, int mb_h, int crop_right, int crop_bottom, int sps_id, int num_ref_frames, int profile_idc,
                             int level_idc, uint8_t *out, size_t cap, size_t *len)
{
    if (len) *len = 0;
    if (!params || !len || (!out && cap) || !sws_params_ok(*params)) return PCAMV_EINVAL;
    const pcamv_stream_params_t &P = *params;
    pcamv_sps_t S = pcamv_sps_t();
    S.profile_idc = profile_idc; S.level_idc = level_idc; S.sps_id = sps_id;
    S.chroma_format_idc = 1; S.bit_depth_luma = 8; S.bit_depth_chroma = 8;
    S.log2_max_frame_num = P.log2_max_frame_num; S.poc_type = P.poc_type; S.log2_max_poc_lsb = P.poc_type == 0 ? P.log2_max_poc_lsb : 0;
    S.delta_pic_order_always_zero = P.poc_type == 1 ? !!P.delta_pic_order_always_zero : 0;
    S.num_ref_frames = num_ref_frames; S.mb_w = mb_w; S.mb_h = mb_h; S.frame_mbs_only = 1; S.direct_8x8_inference = 1;
    S.frame_cropping = crop_right || crop_bottom; S.crop_right = crop_right / 2; S.crop_bottom = crop_bottom / 2;       /* (set.c:139-143, 275-281) */
    pcamv_pps_t Q = pcamv_pps_t();
    Q.pps_id = P.pps_id; Q.sps_id = sps_id; Q.entropy_cabac = !!P.entropy_cabac; Q.pic_order_present = !!P.pic_order_present; Q.num_slice_groups = 1;
    Q.num_ref_idx_l0_default = P.num_ref_idx_l0_default; Q.num_ref_idx_l1_default = 1; Q.weighted_pred = !!P.weighted_pred;
    Q.pic_init_qp = P.pic_init_qp; Q.pic_init_qs = 26; Q.deblocking_filter_control_present = !!P.deblocking_filter_control_present;
    Q.redundant_pic_cnt_present = !!P.redundant_pic_cnt_present;
    uint8_t rs[PCAMV_PSET_RBSP_MAX], rp[PCAMV_PSET_RBSP_MAX];
    const int ns = ps_write_sps(S, rs), np = ps_write_pps(Q, rp);
    if (ns < 0) return ns;
    if (np < 0) return np;
    size_t a = 0, c2 = 0;
    TRY(pcamv_gpu_rbsp_to_nal(rs, (size_t)ns, 3, 7, out, cap, &a));
    TRY(pcamv_gpu_rbsp_to_nal(rp, (size_t)np, 3, 8, out + a, cap - a, &c2));
    *len = a + c2;
    return 0;
}
extern "C" int pcamv_gpu_param_set_head(const pcamv_stream_params_t *params, int mb_w, int mb_h, int sps_id, int num_ref_frames, int profile_idc, int level_idc,
                                        uint8_t *out, size_t cap, size_t *len)
{
    return param_set_head_at(params, mb_w, mb_h, 0, 0, sps_id, num_ref_frames, profile_idc, level_idc, out, cap, len);
}
extern "C" int pcamv_gpu_param_set_head2(const pcamv_stream_params_t *params, int width, int height, int sps_id, int num_ref_frames, int profile_idc, int level_idc,
                                         uint8_t *out, size_t cap, size_t *len)
{
    if (len) *len = 0;
    if (width < 2 || height < 2 || (width & 1) || (height & 1) || width > 16 * SRC_DIM_MAX || height > 16 * SRC_DIM_MAX) return PCAMV_EINVAL;
    const int mb_w = (width + 15) / 16, mb_h = (height + 15) / 16;
    return param_set_head_at(params, mb_w, mb_h, 16 * mb_w - width, 16 * mb_h - height, sps_id, num_ref_frames, profile_idc, level_idc, out, cap, len);
}
extern "C" int pcamv_gpu_debug_slice_records(pcamv_ctx_t *c, pcamv_mb_t *out_mb, int *guard_intact)
{
    if (!c || !out_mb || !c->d_rx_mbs) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const pcamv_mb_t *mbs = c->d_rx_mbs;
    if (c->win && c->win->sw.k_last) {          /* behind a window call: the records of the last slot that took a unit, as its steps would have left them */
        const pcamv_batch *b = c->win;
        long long was = 0, now = 0;
        HIPCHK(c, hipMemcpy(&was, b->sw.d_cursor_was + c->win_i, 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&now, b->sx.d_at + 5 * (size_t)b->sx.n + c->win_i, 8, hipMemcpyDeviceToHost));
        if (now > was && now - was <= b->sw.k_last)
            mbs = b->sw.d_mbs + ((size_t)c->win_i * (size_t)b->sw.k_last + (size_t)(now - was - 1)) * ((size_t)c->F.n_mb + SLICE_GUARD_MBS);
    }
    HIPCHK(c, hipMemcpy(out_mb, mbs, (size_t)c->F.n_mb * sizeof(pcamv_mb_t), hipMemcpyDeviceToHost));
    if (guard_intact) {
        uint8_t g[SLICE_GUARD_MBS * sizeof(pcamv_mb_t)];
        HIPCHK(c, hipMemcpy(g, mbs + c->F.n_mb, sizeof(g), hipMemcpyDeviceToHost));
        *guard_intact = 1;
        for (size_t i = 0; i < sizeof(g); i++) if (g[i] != 0xA5) *guard_intact = 0;
    }
    return 0;
}
/* diff[i] = bits in which context i's received stream differs from its attached payload (payload bits past its end are zeros): the
 * BER numerator of every chain, one kernel over the batch and one copy.  Synchronises. */
extern "C" int pcamv_gpu_batch_payload_check(pcamv_batch_t *b, int64_t *diff)
{
    if (!b || !diff) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    hipStream_t st = b->ctx[0]->stream;
    HIPCHK(b, hipDeviceSynchronize());
    const ExtractDev *dX; int slot;
    TRY(batch_push_xdescs(b, st, &dX, &slot));
    timed_kernel(b, KT_PAYLOAD_CHECK, st, k_payload_check, dim3(b->n), dim3(256), dX, b->d_chk);
    TRY(launched(b));
    TRY(ring_release(b, b->xring, slot, st));
    HIPCHK(b, hipStreamSynchronize(st));
    static_assert(sizeof(long long) == sizeof(int64_t), "payload_check copies the counts as they are");
    HIPCHK(b, hipMemcpy(diff, b->d_chk, sizeof(int64_t) * b->n, hipMemcpyDeviceToHost));
    for (int i = 0; i < b->n; i++) { const int rc = rx_check(b->ctx[i], NULL); if (rc) return fail(b, rc, "context %d: %s", i, b->ctx[i]->err); }
    return 0;
}

/* ------------------------------------------------------------------ one message for the batch (pcamv_message.h, pcamv_message.hip.h) */
extern "C" int pcamv_gpu_message_plan(const int32_t *m, const int32_t *status, int contexts, int k, int64_t capacity, int64_t *state, int64_t *at)
{
    if (!m || !state || !at || contexts < 1 || k < 1) return PCAMV_EINVAL;
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "the caller's arrays are read as they are");
    pcamv_message_plan(m, status, contexts, k, capacity < 0 ? PCAMV_MSG_NO_CAP : capacity, PCAMV_EEOF, (long long *)state, (long long *)at);
    return 0;
}
extern "C" void pcamv_gpu_message_state_reset(int64_t *state, int64_t cursor) { if (state) pcamv_message_state_reset((long long *)state, cursor); }
extern "C" int32_t pcamv_gpu_message_frame_bits(float emrate, int32_t n_carriers) { return pcamv_stc_frame_bits(emrate, n_carriers); }
/* the parity probe: k_message_plan on the caller's arrays, no context's state involved */
extern "C" int pcamv_gpu_message_plan_device(pcamv_ctx_t *c, const int32_t *m, const int32_t *status, int contexts, int k, int64_t capacity, int64_t *state, int64_t *at)
{
    if (!c || !m || !state || !at || contexts < 1 || k < 1 || (long long)contexts * k > (1LL << 24)) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t jobs = (size_t)contexts * (size_t)k;
    DevBuf<int> d_m, d_st; DevBuf<long long> d_state, d_at;
    TRY(d_m.room(c, jobs)); TRY(d_at.room(c, jobs + 1)); TRY(d_state.room(c, MSG_WORDS));
    if (status) TRY(d_st.room(c, jobs));
    HIPCHK(c, hipMemcpy(d_m, m, jobs * 4, hipMemcpyHostToDevice));
    if (status) HIPCHK(c, hipMemcpy(d_st, status, jobs * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_state, state, MSG_WORDS * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(d_at, 0xA5, (jobs + 1) * 8));           /* (the word behind the jobs comes back with them: at[jobs] is the caller's to look at) */
    hipLaunchKernelGGL(k_message_plan, dim3(1), dim3(MSG_PLAN_THREADS), 0, c->stream, d_m, status ? (const int *)d_st : (const int *)NULL, contexts, k,
                       capacity < 0 ? PCAMV_MSG_NO_CAP : (long long)capacity, d_state, d_at, (const EmbedDev *)NULL);
    TRY(launched(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(state, d_state, MSG_WORDS * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(at, d_at, (jobs + 1) * 8, hipMemcpyDeviceToHost));
    return 0;
}
/* Sender */
/* a message can be attached only where no member has another source of bits attached: refused before anything changes */
static int message_members_free(pcamv_batch *b)
{
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        if (c->E.payload) return fail(b, PCAMV_EINVAL, "context %d has a payload of its own attached (pcamv_gpu_set_payload)", i);
        for (int k = 0; k < c->n_member; k++)
            if (c->member_of[k] != b && c->member_of[k]->d_msg) return fail(b, PCAMV_EINVAL, "context %d belongs to another batch that has a message attached", i);
    }
    return 0;
}
static int message_attach(pcamv_batch *b, const uint8_t *d_bytes, int64_t n_bits, int64_t start_bit)
{
    if (d_bytes) {
        TRY(b->d_mtx.room(b, MSG_WORDS)); TRY(b->d_mtx_m.room(b, (size_t)b->n)); TRY(b->d_mtx_at.room(b, (size_t)b->n));      /* (made by the first message) */
        long long st[MSG_WORDS];
        pcamv_message_state_reset(st, start_bit);
        HIPCHK(b, hipMemcpy(b->d_mtx, st, sizeof(st), hipMemcpyHostToDevice));
    }
    b->d_msg = d_bytes; b->msg_bits = d_bytes ? n_bits : 0;
    return 0;
}
extern "C" int pcamv_gpu_batch_set_message(pcamv_batch_t *b, const uint8_t *bytes, int64_t n_bits, int64_t start_bit)
{
    if (!b || n_bits < 0 || start_bit < 0) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    HIPCHK(b, hipDeviceSynchronize());          /* frames in flight still read the message attached so far */
    if (!bytes || !n_bits) return message_attach(b, NULL, 0, 0);
    TRY(message_members_free(b));
    const size_t nb = (size_t)((n_bits + 7) >> 3);
    b->d_msg = NULL;                            /* (detached until the new bytes stand) */
    TRY(b->d_msg_own.room(b, nb));
    HIPCHK(b, hipMemcpy(b->d_msg_own, bytes, nb, hipMemcpyHostToDevice));
    return message_attach(b, b->d_msg_own, n_bits, start_bit);
}
extern "C" int pcamv_gpu_batch_set_message_device(pcamv_batch_t *b, const void *d_bytes, int64_t n_bits, int64_t start_bit)
{
    if (!b || n_bits < 0 || start_bit < 0) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    HIPCHK(b, hipDeviceSynchronize());
    if (d_bytes && n_bits) TRY(message_members_free(b));
    return message_attach(b, d_bytes && n_bits ? (const uint8_t *)d_bytes : NULL, n_bits, start_bit);
}
extern "C" int pcamv_gpu_batch_message_tell(pcamv_batch_t *b, int64_t *next_bit, int64_t *n_bits)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    if (!b->d_msg) return fail(b, PCAMV_EINVAL, "no message is attached to this batch (pcamv_gpu_batch_set_message)");
    HIPCHK(b, hipDeviceSynchronize());
    long long cur = 0;
    HIPCHK(b, hipMemcpy(&cur, b->d_mtx + MSG_CURSOR, sizeof(cur), hipMemcpyDeviceToHost));
    if (next_bit) *next_bit = cur;
    if (n_bits) *n_bits = b->msg_bits;
    return 0;
}
/* Receiver */
extern "C" int pcamv_gpu_batch_rx_message_reset(pcamv_batch_t *b)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    if (!b->d_mrx) return fail(b, PCAMV_EINVAL, "this batch has no reservation (pcamv_gpu_batch_rx_message_reserve)");
    HIPCHK(b, hipDeviceSynchronize());
    long long st[MSG_WORDS];
    pcamv_message_state_reset(st, 0);
    HIPCHK(b, hipMemcpy(b->d_mrx_state, st, sizeof(st), hipMemcpyHostToDevice));
    HIPCHK(b, hipMemset(b->d_mrx, 0, (size_t)((b->mrx_bits + 31) >> 5) * 4));
    const long long lcg = 1;                    /* every context's column generator at its initial state; its own stream stays as it is */
    for (int i = 0; i < b->n; i++) HIPCHK(b, hipMemcpy(b->ctx[i]->E.pstate + PST_RX_LCG, &lcg, sizeof(lcg), hipMemcpyHostToDevice));
    return 0;
}
extern "C" int pcamv_gpu_batch_rx_message_reserve(pcamv_batch_t *b, int64_t n_bits)
{
    if (!b || n_bits < 0) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    HIPCHK(b, hipDeviceSynchronize());
    b->d_mrx.release(); b->mrx_bits = 0;        /* (a reservation is a buffer of its own size: while there is none, d_mrx is NULL) */
    if (!n_bits) return 0;
    const size_t jobs = (size_t)b->n * PCAMV_STREAM_WINDOW_MAX;
    TRY(b->d_mrx_state.room(b, MSG_WORDS)); TRY(b->d_mrx_job.room(b, 2 * jobs)); TRY(b->d_mrx_at.room(b, jobs));     /* (made by the first reservation) */
    TRY(b->d_mchk.room(b, MSG_CHECK_GROUPS + 1));
    const size_t words = (size_t)((n_bits + 31) >> 5);
    TRY(b->d_mrx.room(b, words + MSG_GUARD_WORDS));                 /* guard words behind the stream that nothing may write (pcamv_gpu_batch_debug_rx_message_guard) */
    HIPCHK(b, hipMemset(b->d_mrx + words, 0xA5, MSG_GUARD_WORDS * 4));
    b->mrx_bits = n_bits;
    const int rc = pcamv_gpu_batch_rx_message_reset(b);
    if (rc) { b->d_mrx.release(); b->mrx_bits = 0; }
    return rc;
}
/* synchronises; are the guard words behind the batch's received stream as the reservation left them? */
extern "C" int pcamv_gpu_batch_debug_rx_message_guard(pcamv_batch_t *b, int *guard_intact)
{
    if (!b || !guard_intact || !b->d_mrx) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    HIPCHK(b, hipDeviceSynchronize());
    uint8_t g[MSG_GUARD_WORDS * 4];
    HIPCHK(b, hipMemcpy(g, b->d_mrx + (size_t)((b->mrx_bits + 31) >> 5), sizeof(g), hipMemcpyDeviceToHost));
    *guard_intact = 1;
    for (size_t i = 0; i < sizeof(g); i++) if (g[i] != 0xA5) *guard_intact = 0;
    return 0;
}
/* after a synchronisation: the state words; did a frame run past the batch's reservation?  (reported once, like rx_check) */
static int rx_message_check(pcamv_batch *b, long long *st)
{
    if (!b->d_mrx) return fail(b, PCAMV_EINVAL, "this batch has no reservation (pcamv_gpu_batch_rx_message_reserve)");
    HIPCHK(b, hipDeviceSynchronize());
    HIPCHK(b, hipMemcpy(st, b->d_mrx_state, MSG_WORDS * sizeof(long long), hipMemcpyDeviceToHost));
    if (st[MSG_OVERRUN]) {
        hipMemset(b->d_mrx_state + MSG_OVERRUN, 0, sizeof(long long));
        return fail(b, PCAMV_ENOMEM, "received message: %lld bits extracted, %lld reserved (the bits beyond were dropped)", st[MSG_CURSOR], b->mrx_bits);
    }
    return 0;
}
extern "C" int pcamv_gpu_batch_rx_message_tell(pcamv_batch_t *b, int64_t *received_bits, int64_t *reserved_bits, int64_t *valid_bits, int64_t first_bad[3])
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    long long st[MSG_WORDS] = {0};
    const int rc = rx_message_check(b, st);
    if (rc && rc != PCAMV_ENOMEM) return rc;
    if (received_bits) *received_bits = st[MSG_CURSOR];
    if (reserved_bits) *reserved_bits = b->mrx_bits;
    if (valid_bits) *valid_bits = st[MSG_VALID] < 0 ? st[MSG_CURSOR] : st[MSG_VALID];
    if (first_bad) { first_bad[0] = st[MSG_BAD_CALL]; first_bad[1] = st[MSG_BAD_SLOT]; first_bad[2] = st[MSG_BAD_CTX]; }
    return rc;
}
extern "C" int pcamv_gpu_batch_rx_message_fetch(pcamv_batch_t *b, uint8_t *bytes, int64_t n_bits)
{
    if (!b || !bytes || n_bits < 0 || n_bits > b->mrx_bits) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    long long st[MSG_WORDS];
    TRY(rx_message_check(b, st));
    if (n_bits) HIPCHK(b, hipMemcpy(bytes, b->d_mrx, (size_t)((n_bits + 7) >> 3), hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int pcamv_gpu_batch_message_check(pcamv_batch_t *b, int64_t *diff, int64_t *received_bits, int64_t *valid_bits)
{
    if (!b || !diff) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    if (!b->d_msg) return fail(b, PCAMV_EINVAL, "no message is attached to this batch (pcamv_gpu_batch_set_message)");
    long long state[MSG_WORDS];
    TRY(rx_message_check(b, state));
    hipStream_t st = b->ctx[0]->stream;
    long long got = state[MSG_CURSOR] < b->mrx_bits ? state[MSG_CURSOR] : b->mrx_bits;
    long long groups = (((got + 7) >> 3) + 255) / 256;
    groups = groups < 1 ? 1 : groups > MSG_CHECK_GROUPS ? MSG_CHECK_GROUPS : groups;
    timed(b, KT_MESSAGE_CHECK, st, [&] {        /* (the two kernels of a check under one timer) */
        hipLaunchKernelGGL(k_message_check, dim3((unsigned)groups), dim3(256), 0, st, (const uint8_t *)b->d_mrx.p, b->mrx_bits, b->d_mrx_state, b->d_msg, b->msg_bits, b->d_mchk);
        hipLaunchKernelGGL(k_message_check_sum, dim3(1), dim3(256), 0, st, b->d_mchk, (int)groups, b->d_mchk + MSG_CHECK_GROUPS);
    });
    TRY(launched(b));
    HIPCHK(b, hipStreamSynchronize(st));
    static_assert(sizeof(long long) == sizeof(int64_t), "message_check copies the count as it is");
    HIPCHK(b, hipMemcpy(diff, b->d_mchk + MSG_CHECK_GROUPS, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (received_bits) *received_bits = state[MSG_CURSOR];
    if (valid_bits) *valid_bits = state[MSG_VALID] < 0 ? state[MSG_CURSOR] : state[MSG_VALID];
    return 0;
}

/* ------------------------------------------------------------------ sender to a stream (k_write_pslice, k_write_pslice_cavlc; pcamv_slice.hip.h) */
static int write_header_ok(const pcamv_slice_hdr_t *h)
{
    return h->n_bits >= 0 && h->n_bits <= (1 << 24) && (!h->n_bits || h->bits) && h->nal_ref_idc >= 0 && h->nal_ref_idc <= 3 && h->nal_unit_type >= 0 && h->nal_unit_type <= 31;
}
/* what every launch of a writer needs of the batch, once its mode is the contexts' and each of them has a frame to write (a batch is of
 * one mode, pcamv_gpu_batch_create: the first context decides the mode check, so it may run for all before the frames are looked at) */
static int write_setup(pcamv_batch *b, int cavlc)
{
    TRY(entropy_mode(b, cavlc, "pcamv_gpu_write_pslice_cavlc and pcamv_gpu_batch_write_step_cavlc write", "pcamv_gpu_write_pslice and pcamv_gpu_batch_write_step write"));
    for (int i = 0; i < b->n; i++) if (!b->ctx[i]->last) return fail(b, PCAMV_EINVAL, "context %d has analysed no frame yet: there is nothing to write", i);
    return entropy_setup(b, b->d_wstat, b->d_sw_tab, b->d_sw_scratch, cavlc, SW_NCTX);
}
/* the callers' headers into the next staging buffer -- n_hdr entries of SW_HDR_WORDS words, then the bits of each at a multiple of
 * 4 -- with one copy on `st`; *stage_out is released (stage_release) once the kernel that reads it is queued */
static int write_stage(pcamv_batch *b, const pcamv_slice_hdr_t *hdrs, int n_hdr, hipStream_t st, const int **d_hdr, int *stage_out)
{
    static const pcamv_slice_hdr_t none = {NULL, 0, 0, 2, 1};
    if (!hdrs) { hdrs = &none; n_hdr = 1; }
    size_t total = (size_t)n_hdr * SW_HDR_WORDS * 4;
    for (int i = 0; i < n_hdr; i++) {
        if (!write_header_ok(&hdrs[i])) return fail(b, PCAMV_EINVAL, "slice header %d: bits missing, n_bits, nal_ref_idc or nal_unit_type out of range", i);
        total += ((size_t)(hdrs[i].n_bits + 7) / 8 + 3) & ~(size_t)3;
    }
    int k;
    TRY(stage_take(b, b->tx_stage, total, &k));
    uint8_t *h = b->tx_stage.h[k];
    int *w = (int *)h;
    size_t at = (size_t)n_hdr * SW_HDR_WORDS * 4;
    for (int i = 0; i < n_hdr; i++) {
        const size_t nb = (size_t)(hdrs[i].n_bits + 7) / 8;
        w[SW_HDR_WORDS * i] = (int)at; w[SW_HDR_WORDS * i + 1] = hdrs[i].n_bits; w[SW_HDR_WORDS * i + 2] = hdrs[i].i_frame;
        w[SW_HDR_WORDS * i + 3] = hdrs[i].nal_ref_idc << 5 | hdrs[i].nal_unit_type;
        if (nb) memcpy(h + at, hdrs[i].bits, nb);
        at += (nb + 3) & ~(size_t)3;
    }
    TRY(stage_send(b, b->tx_stage, k, total, st));
    *d_hdr = (const int *)b->tx_stage.d[k].p; *stage_out = k;
    return 0;
}
/* one launch over the batch's contexts as they stand: J brings the destination and the mode.  The headers are the host's (hdrs, staged
 * here), or with sw a header table on the device that k_stream_slot fills in front of the writer from the descriptors the writer reads;
 * k_stream_commit then follows the writer */
static int write_run(pcamv_batch *b, WriteJobs J, const pcamv_slice_hdr_t *hdrs, int n_hdr, int cavlc, hipStream_t st, const StreamWrite *sw = NULL)
{
    int k = -1;
    if (sw) { J.hdr = sw->table; J.n_hdr = b->n; }
    else {
        TRY(write_stage(b, hdrs, n_hdr, st, &J.hdr, &k));
        J.n_hdr = hdrs ? n_hdr : 1;
    }
    J.status = b->d_wstat; J.tab = b->d_sw_tab; J.scratch = b->d_sw_scratch; J.scratch_stride = (long long)row_bytes(b, cavlc);
    J.lds_cols = b->sp_lds_cols;
    const FrameDev *dF; const EmbedDev *dE; int slot;
    int rc = batch_push_descs(b, st, &dF, &dE, &slot);
    if (!rc) {
        if (sw) timed_kernel(b, KT_STREAM_SLOT, st, k_stream_slot, dim3((b->n + 63) / 64), dim3(64), dF, *sw);
        if (cavlc) timed(b, KT_WRITE_PSLICE_CAVLC, st, [&] { pcamv_launch_write_pslice_cavlc((unsigned)b->n, st, dF, J); });
        else timed(b, KT_WRITE_PSLICE, st, [&] { pcamv_launch_write_pslice((unsigned)b->n, st, dF, J); });
        if (sw) timed_kernel(b, KT_STREAM_COMMIT, st, k_stream_commit, dim3((b->n + 63) / 64), dim3(64), *sw);
        if (sw && b->rate_open) rate_launch(b, 0, st);
        rc = launched(b);
        if (!rc) rc = ring_release(b, b->ring, slot, st);
    }
    const int rc2 = k >= 0 ? stage_release(b, b->tx_stage, k, st) : 0;     /* released on every path */
    return rc ? rc : rc2;
}
/* Every context's last step as a CABAC (cavlc: CAVLC) P slice, final motion (the records with the flip map of the step's embedding stage), from one
 * launch on `stream`, no host synchronisation.
 * Ordering is the caller's, as for pcamv_gpu_batch_extract_slices_device (the borrowed buffer and the three arrays belong to `stream`'s
 * timeline), and the call belongs after the batch_step whose frame it writes and before the next one: the kernel reads that step's
 * source planes (fenc), padded reference planes, records, flip map and carrier index.  Within a step the stages run in the order
 * planes, analysis, embedding, second pass (batch_launch); the analysis writes records, reconstruction and motion field, the
 * embedding the flip map, the second pass reconstruction, motion field and non-zero flags in place -- none of which the writer reads
 * but the records and the flip map, both complete when the step is.  The first thing of the NEXT step to overwrite anything read here is
 * its plane stage (k_hpel / k_chroma_pad: the padded planes), then its analysis (the records); the source planes are the caller's and
 * stay until the caller replaces them. */
static int batch_write_step(pcamv_batch_t *b, const pcamv_slice_hdr_t *hdrs, int n_hdr, int as_nal, void *bytes, size_t bytes_size,
                            const int64_t *off, const int64_t *cap, int64_t *len, int cavlc, void *stream)
{
    if (!b || !bytes || !off || !cap || !len || bytes_size > ((size_t)1 << 62)) return PCAMV_EINVAL;
    if (hdrs ? (n_hdr != 1 && n_hdr != b->n) : n_hdr != 0) return fail(b, PCAMV_EINVAL, "n_hdr is 1 or the batch size (0 with no header)");
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    TRY(write_setup(b, cavlc));
    static_assert(sizeof(long long) == sizeof(int64_t), "the caller's int64 arrays are read as they are");
    WriteJobs J = {};
    J.bytes = (uint8_t *)bytes; J.bytes_size = (long long)bytes_size;
    J.off = (const long long *)off; J.cap = (const long long *)cap; J.len = (long long *)len;
    J.mbs = NULL; J.as_nal = as_nal != 0; J.final = 1;
    return write_run(b, J, hdrs, n_hdr, cavlc, stream ? (hipStream_t)stream : b->ctx[0]->stream);
}
extern "C" int pcamv_gpu_batch_write_step(pcamv_batch_t *b, const pcamv_slice_hdr_t *hdrs, int n_hdr, int as_nal, void *bytes, size_t bytes_size,
                                          const int64_t *off, const int64_t *cap, int64_t *len, void *stream)
{
    return batch_write_step(b, hdrs, n_hdr, as_nal, bytes, bytes_size, off, cap, len, 0, stream);
}
/* the same as a CAVLC P slice (k_write_pslice_cavlc), for contexts opened with --no-cabac */
extern "C" int pcamv_gpu_batch_write_step_cavlc(pcamv_batch_t *b, const pcamv_slice_hdr_t *hdrs, int n_hdr, int as_nal, void *bytes, size_t bytes_size,
                                                const int64_t *off, const int64_t *cap, int64_t *len, void *stream)
{
    return batch_write_step(b, hdrs, n_hdr, as_nal, bytes, bytes_size, off, cap, len, 1, stream);
}
/* synchronises; status[i] = return code of context i's slice in the last write call (0 or PCAMV_ENOMEM; PCAMV_EINVAL for a place
 * outside the buffer) */
extern "C" int pcamv_gpu_batch_write_status(pcamv_batch_t *b, int32_t *status)
{
    return status_fetch(b, &pcamv_batch::d_wstat, status, "this batch has written no slices yet");
}
/* A capacity under which no slice of the context's picture size fails: SW_MB_BOUND bytes per macroblock (derived in
 * pcamv_slice_write.h from the most bits a decision, a level and an mvd can take), the header's bytes, the flush; as a NAL unit
 * start code and header byte, and one emulation prevention byte for every two bytes of RBSP at the worst (each takes two zeros
 * before it and resets the count). */
extern "C" int64_t pcamv_gpu_slice_bound(const pcamv_ctx_t *c, int32_t hdr_bits, int as_nal)
{
    if (!c || hdr_bits < 0) return PCAMV_EINVAL;
    const int64_t rbsp = (int64_t)SW_MB_BOUND * c->F.n_mb + (hdr_bits + 7) / 8 + SW_TAIL_BOUND;
    return as_nal ? 5 + rbsp + rbsp / 2 + 1 : rbsp;
}
/* the parity probe: one slice of the context's last frame (mbs == NULL; final: with the embedding stage's flip map) or of uploaded
 * records that hold final motion, written on the device, copied back.  Synchronises. */
static int write_pslice(pcamv_ctx_t *c, const pcamv_slice_hdr_t *hdr, int final, const pcamv_mb_t *mbs, int as_nal, uint8_t *out, size_t cap, size_t *len,
                        int cavlc)
{
    if (!c || !out || !len || cap > ((size_t)1 << 40)) return PCAMV_EINVAL;
    *len = 0;
    HIPCHK(c, hipSetDevice(c->device));
    pcamv_batch *b = c->self;
    TRY(on_behalf(c, b, batch_live(b)));
    TRY(on_behalf(c, b, write_setup(b, cavlc)));
    if (mbs) {
        TRY(rx_mbs(c));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(c->d_rx_mbs, mbs, (size_t)c->F.n_mb * sizeof(pcamv_mb_t), hipMemcpyHostToDevice));
    }
    DevBuf<uint8_t> d_out;      /* [off][cap][len] int64, then the slice */
    const size_t arr = 3 * sizeof(long long);
    TRY(d_out.room(c, arr + (cap ? cap : 1)));
    const long long h_arr[3] = {0, (long long)cap, 0};
    int st = 0;
    long long n = 0;
    HIPCHK(c, hipMemcpy(d_out, h_arr, arr, hipMemcpyHostToDevice));
    WriteJobs J = {};
    J.bytes = d_out + arr; J.bytes_size = (long long)cap;
    J.off = (const long long *)d_out.p; J.cap = J.off + 1; J.len = (long long *)d_out.p + 2;
    J.mbs = mbs ? c->d_rx_mbs : NULL; J.as_nal = as_nal != 0; J.final = final != 0;
    TRY(on_behalf(c, b, write_run(b, J, hdr, hdr ? 1 : 0, cavlc, c->stream)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&st, b->d_wstat, sizeof(st), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&n, J.len, sizeof(n), hipMemcpyDeviceToHost));
    if (!st && n > 0 && (size_t)n <= cap) HIPCHK(c, hipMemcpy(out, J.bytes, (size_t)n, hipMemcpyDeviceToHost));
    if (st) return fail(c, st, st == PCAMV_ENOMEM ? "the slice does not fit %zu bytes (pcamv_gpu_slice_bound gives a capacity that always does)" :
                        "the records are no P macroblocks of this path (type, partition or sub-partition out of range)", cap);
    if (n < 0 || (size_t)n > cap) return fail(c, PCAMV_EHIP, "write_pslice: length corrupt");
    *len = (size_t)n;
    return 0;
}
extern "C" int pcamv_gpu_write_pslice(pcamv_ctx_t *c, const pcamv_slice_hdr_t *hdr, int final, const pcamv_mb_t *mbs, int as_nal, uint8_t *out, size_t cap,
                                      size_t *len)
{
    return write_pslice(c, hdr, final, mbs, as_nal, out, cap, len, 0);
}
extern "C" int pcamv_gpu_write_pslice_cavlc(pcamv_ctx_t *c, const pcamv_slice_hdr_t *hdr, int final, const pcamv_mb_t *mbs, int as_nal, uint8_t *out, size_t cap,
                                            size_t *len)
{
    return write_pslice(c, hdr, final, mbs, as_nal, out, cap, len, 1);
}
/* the inverse of pcamv_gpu_nal_to_rbsp, as x264_nal_encode writes a unit (common/common.c:658-695): long start code, header byte, the
 * RBSP with an emulation prevention byte before every byte <= 3 that follows two zeros.  Host code. */
extern "C" int pcamv_gpu_rbsp_to_nal(const uint8_t *rbsp, size_t len, int nal_ref_idc, int nal_unit_type, uint8_t *nal, size_t cap, size_t *nal_len)
{
    if ((!rbsp && len) || !nal || !nal_len || nal_ref_idc < 0 || nal_ref_idc > 3 || nal_unit_type < 0 || nal_unit_type > 31) return PCAMV_EINVAL;
    size_t n = 0;
    int zeros = 0;
    const uint8_t head[5] = {0, 0, 0, 1, (uint8_t)(nal_ref_idc << 5 | nal_unit_type)};
    *nal_len = 0;
    for (int i = 0; i < 5; i++) { if (n >= cap) return PCAMV_ENOMEM; nal[n++] = head[i]; }
    for (size_t i = 0; i < len; i++) {
        if (zeros == 2 && rbsp[i] <= 3) { if (n >= cap) return PCAMV_ENOMEM; nal[n++] = 3; zeros = 0; }
        zeros = rbsp[i] == 0 ? zeros + 1 : 0;
        if (n >= cap) return PCAMV_ENOMEM;
        nal[n++] = rbsp[i];
    }
    *nal_len = n;
    return 0;
}

/* ------------------------------------------------------------------ sender to byte streams (k_stream_open, k_stream_slot, k_stream_commit; pcamv_stream_write.h) */
extern "C" int pcamv_gpu_write_slice_header(const pcamv_stream_params_t *params, const pcamv_slice_fields_t *fields, uint8_t *bits, size_t cap, int32_t *n_bits)
{
    if (n_bits) *n_bits = 0;
    if (!params || !fields || !n_bits || (!bits && cap)) return PCAMV_EINVAL;
    int n = 0;
    TRY(pcamv_slice_header_write(*params, *fields, NULL, &n));          /* judged and counted; nothing stored */
    if ((size_t)(n + 7) / 8 > cap) return PCAMV_ENOMEM;
    const int rc = pcamv_slice_header_write(*params, *fields, bits, &n);
    *n_bits = n;
    return rc;
}
/* the arrays of the library's block for n contexts (StreamOut::d_own), every one at a multiple of 8 */
static size_t stream_out_bytes(int n) { return (size_t)n * (sizeof(SwsCtx) + 5 * 8 + 4 + SWS_HDR_WORDS * 4 + PCAMV_SLICE_HDR_BYTES) + 8; }
/* ... and of the block of a copy launch (StreamOut::d_copy; stream_copy_jobs below) */
static size_t stream_copy_bytes(int n) { return (size_t)n * (sizeof(VcJob) + 3 * 8) + 8 + 8; }
static StreamWrite stream_out_jobs(const pcamv_batch *b)
{
    const StreamOut &O = b->so;
    const size_t n = (size_t)b->n;
    static_assert(sizeof(SwsCtx) % 8 == 0, "the int64 arrays follow the contexts' states");
    StreamWrite J = StreamWrite();
    J.bytes = O.bytes; J.bytes_size = O.bytes_size; J.len = O.len;
    J.ctx = (SwsCtx *)O.d_own.p;
    J.w_off = (long long *)(J.ctx + n); J.w_cap = J.w_off + n; J.w_len = J.w_cap + n;
    long long *at = J.w_len + n;
    J.off = at; J.cap = at + n;
    J.first = (int *)(at + 2 * n); J.table = J.first + ((n + 1) & ~(size_t)1);
    J.status = b->d_wstat; J.head = O.d_head; J.S = O.S; J.n = b->n;
    return J;
}
extern "C" int pcamv_gpu_batch_stream_open(pcamv_batch_t *b, void *bytes, size_t bytes_size, const int64_t *off, const int64_t *cap, int64_t *len,
                                           const pcamv_stream_params_t *params, const pcamv_stream_write_t *wr, const uint8_t *head, size_t head_len, void *stream)
{
    if (!b || !bytes || !off || !cap || !len || !params || !wr || (!head && head_len) || head_len > ((size_t)1 << 24) || bytes_size > ((size_t)1 << 62)) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    SwsSetup S; S.P = *params; S.W = *wr;
    const int ok = sws_setup_ok(S);
    if (ok == PCAMV_EUNSUP) return fail(b, ok, "weighted prediction: the header writer has no pred_weight_table");
    if (ok) return fail(b, ok, wr->nal_ref_idc == 0 ? "nal_ref_idc 0: in this path a chain's P frame is the next one's reference" :
                               "stream_open: parameter sets or stream settings out of range");
    if (b->rate_open) return fail(b, PCAMV_EINVAL, "a rate is open on this batch's streams: pcamv_gpu_batch_rate_close first");
    StreamOut &O = b->so;
    O.ready = 0; O.joined = 0; O.stepped = 0;
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    const size_t total = stream_out_bytes(b->n);
    if (total > O.d_own.cap || head_len > O.d_head.cap || stream_copy_bytes(b->n) > O.d_copy.cap) HIPCHK(b, hipDeviceSynchronize());        /* (steps on the blocks that are replaced may be in flight) */
    TRY(O.d_own.room(b, total));
    TRY(O.d_head.room(b, head_len));
    TRY(O.d_copy.room(b, stream_copy_bytes(b->n)));        /* (what a join behind this open works in) */
    O.bytes = (uint8_t *)bytes; O.bytes_size = (long long)bytes_size; O.len = (long long *)len; O.S = S;
    StreamWrite J = stream_out_jobs(b);
    static_assert(sizeof(long long) == sizeof(int64_t), "the caller's int64 arrays are read as they are");
    HIPCHK(b, hipMemcpyAsync((void *)J.off, off, 8 * (size_t)b->n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemcpyAsync((void *)J.cap, cap, 8 * (size_t)b->n, hipMemcpyDeviceToDevice, st));
    if (head_len) HIPCHK(b, hipMemcpyAsync(O.d_head, head, head_len, hipMemcpyHostToDevice, st));
    HIPCHK(b, hipStreamSynchronize(st));                                /* off, cap and head are read by this call alone: copied on return */
    J.head_len = (long long)head_len;
    timed_kernel(b, KT_STREAM_OPEN, st, k_stream_open, dim3((b->n + 63) / 64), dim3(64), J);
    TRY(launched(b));
    O.ready = 1;
    return 0;
}
/* ---- a head per context, and the streams joined into one video (k_stream_open_heads, k_stream_join, k_stream_copy_plan, k_stream_copy;
 * pcamv_video.h).  The arrays of a copy launch in the library's block StreamOut::d_copy, every one at a multiple of 8 */
static CopyJobs stream_copy_jobs(const pcamv_batch *b, const uint8_t *src, uint8_t *dst)
{
    static_assert(sizeof(VcJob) % 8 == 0, "the int64 arrays follow the jobs");
    const CopyJobs C = {src, dst, (VcJob *)b->so.d_copy.p, (long long *)((VcJob *)b->so.d_copy.p + b->n), b->n};
    return C;
}
static long long *stream_copy_heads(const pcamv_batch *b) { return stream_copy_jobs(b, NULL, NULL).chunk_base + b->n + 1; }     /* [head_off n][head_len n] */
static int *stream_join_word(const pcamv_batch *b) { return (int *)(stream_copy_heads(b) + 2 * (size_t)b->n); }
/* the plan and the copy behind the kernel that made the jobs; no job holds more than `most` bytes in all, which is what the host knows */
static void stream_copy_launch(pcamv_batch *b, const CopyJobs &C, unsigned long long most, hipStream_t st)
{
    unsigned long long waves = most / VC_CHUNK + 2ULL * (unsigned)C.n + 1;
    if (waves > (1u << 16)) waves = 1u << 16;      /* (a wavefront then takes several chunks in turn) */
    timed_kernel(b, KT_STREAM_COPY_PLAN, st, k_stream_copy_plan, dim3(1), dim3(64), C);
    timed_kernel(b, KT_STREAM_COPY, st, k_stream_copy, dim3((unsigned)waves), dim3(64), C);
}
static int ranges_overlap(const void *a, size_t a_size, const void *b, size_t b_size)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a_size && b_size && a0 < b0 + b_size && b0 < a0 + a_size;
}
extern "C" int pcamv_gpu_batch_stream_open_heads(pcamv_batch_t *b, void *bytes, size_t bytes_size, const int64_t *off, const int64_t *cap, int64_t *len,
                                                 const pcamv_stream_params_t *params, const pcamv_stream_write_t *wr, const void *heads, size_t heads_size,
                                                 const int64_t *head_off, const int64_t *head_len, void *stream)
{
    if (!b || !bytes || !off || !cap || !len || !params || !wr || !heads || !head_off || !head_len || heads_size > ((size_t)1 << 40) ||
        bytes_size > ((size_t)1 << 62) || ranges_overlap(bytes, bytes_size, heads, heads_size)) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    SwsSetup S; S.P = *params; S.W = *wr;
    const int ok = sws_setup_ok(S);
    if (ok == PCAMV_EUNSUP) return fail(b, ok, "weighted prediction: the header writer has no pred_weight_table");
    if (ok) return fail(b, ok, wr->nal_ref_idc == 0 ? "nal_ref_idc 0: in this path a chain's P frame is the next one's reference" :
                               "stream_open_heads: parameter sets or stream settings out of range");
    if (b->rate_open) return fail(b, PCAMV_EINVAL, "a rate is open on this batch's streams: pcamv_gpu_batch_rate_close first");
    StreamOut &O = b->so;
    O.ready = 0; O.joined = 0; O.stepped = 0;
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    const size_t total = stream_out_bytes(b->n), n = (size_t)b->n;
    if (total > O.d_own.cap || stream_copy_bytes(b->n) > O.d_copy.cap) HIPCHK(b, hipDeviceSynchronize());   /* (steps on the blocks that are replaced may be in flight) */
    TRY(O.d_own.room(b, total));
    TRY(O.d_copy.room(b, stream_copy_bytes(b->n)));
    O.bytes = (uint8_t *)bytes; O.bytes_size = (long long)bytes_size; O.len = (long long *)len; O.S = S;
    StreamWrite J = stream_out_jobs(b);
    const CopyJobs C = stream_copy_jobs(b, (const uint8_t *)heads, O.bytes);
    long long *h_at = stream_copy_heads(b);
    HIPCHK(b, hipMemcpyAsync((void *)J.off, off, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemcpyAsync((void *)J.cap, cap, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemcpyAsync(h_at, head_off, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipMemcpyAsync(h_at + n, head_len, 8 * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(b, hipStreamSynchronize(st));                                /* the four arrays are read by this call alone: copied on return */
    const HeadJobs H = {(long long)heads_size, h_at, h_at + n, C.jobs};
    timed_kernel(b, KT_STREAM_OPEN_HEADS, st, k_stream_open_heads, dim3((b->n + 63) / 64), dim3(64), J, H);
    /* the regions do not overlap, so the heads that are taken hold no more than the buffer; each no more than `heads` and VC_HEAD_MAX */
    const unsigned long long each = heads_size < (size_t)VC_HEAD_MAX ? heads_size : (unsigned long long)VC_HEAD_MAX, all = each * n;
    stream_copy_launch(b, C, all < bytes_size ? all : bytes_size, st);
    TRY(launched(b));
    O.ready = 1;
    return 0;
}
extern "C" int pcamv_gpu_batch_join_streams(pcamv_batch_t *b, void *video, size_t video_size, const int64_t *video_off, int64_t *video_len, int64_t *placed,
                                            void *stream)
{
    if (!b || !video || !video_off || !video_len || video_size > ((size_t)1 << 40)) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    StreamOut &O = b->so;
    if (!O.ready) return fail(b, PCAMV_EINVAL, "no byte streams were opened on this batch yet (pcamv_gpu_batch_stream_open*)");
    if (O.bytes_size > (1LL << 40)) return fail(b, PCAMV_EINVAL, "join_streams: the open buffer holds more than 2^40 bytes");
    if (ranges_overlap(video, video_size, O.bytes, (size_t)O.bytes_size)) return fail(b, PCAMV_EINVAL, "join_streams: the video overlaps the buffer the streams are written to");
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    const CopyJobs C = stream_copy_jobs(b, O.bytes, (uint8_t *)video);
    const JoinJobs Q = {(const SwsCtx *)O.d_own.p, b->n, (long long)video_size, (const long long *)video_off, (long long *)video_len, (long long *)placed,
                        stream_join_word(b), C.jobs};
    timed_kernel(b, KT_STREAM_JOIN, st, k_stream_join, dim3(1), dim3(64), Q);
    stream_copy_launch(b, C, (unsigned long long)O.bytes_size < video_size ? (unsigned long long)O.bytes_size : video_size, st);
    TRY(launched(b));
    O.joined = 1;
    return 0;
}
/* synchronises */
extern "C" int pcamv_gpu_batch_join_status(pcamv_batch_t *b)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    if (!b->so.ready || !b->so.joined) return fail(b, PCAMV_EINVAL, "no streams were joined on this batch since its last open (pcamv_gpu_batch_join_streams)");
    HIPCHK(b, hipDeviceSynchronize());
    int rc = 0;
    HIPCHK(b, hipMemcpy(&rc, stream_join_word(b), sizeof(rc), hipMemcpyDeviceToHost));
    return rc ? fail(b, rc, "join_streams: the streams do not fit what is left of the video buffer") : 0;
}
extern "C" int pcamv_gpu_batch_write_stream_step(pcamv_batch_t *b, void *stream)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    if (!b->so.ready) return fail(b, PCAMV_EINVAL, "no byte streams were opened on this batch yet (pcamv_gpu_batch_stream_open)");
    const int cavlc = !b->so.S.P.entropy_cabac;
    TRY(write_setup(b, cavlc));
    const StreamWrite SJ = stream_out_jobs(b);
    WriteJobs J = {};
    J.bytes = SJ.bytes; J.bytes_size = SJ.bytes_size;
    J.off = SJ.w_off; J.cap = SJ.w_cap; J.len = SJ.w_len;
    J.mbs = NULL; J.as_nal = 1; J.final = 1;
    b->so.stepped = 1;
    return write_run(b, J, NULL, 0, cavlc, stream ? (hipStream_t)stream : b->ctx[0]->stream, &SJ);
}
/* ------------------------------------------------------------------ IDR pictures coded on the device (k_idr_mb, k_idr_prefix, k_idr_pack, k_idr_slot, k_idr_unit; pcamv_idr.hip) */
void pcamv_launch_idr_mb(const IdrJobs &J, int g0, int g, int mb_w, int mb_h, hipStream_t st);
void pcamv_launch_idr_mb4(const IdrJobs &J, int g0, int g, int mb_w, int mb_h, hipStream_t st);
void pcamv_launch_idr_prefix(const IdrJobs &J, int g0, int g, hipStream_t st);
void pcamv_launch_idr_pack(const IdrJobs &J, int g0, int g, hipStream_t st);
void pcamv_launch_idr_unit(const IdrJobs &J, int g0, int g, hipStream_t st);
void pcamv_launch_idr_slot(const IdrJobs &J, const void *sws_ctx, int n, hipStream_t st);
void pcamv_launch_idr_deblock(const IdrJobs &J, int n, int mb_w, int mb_h, hipStream_t st);
int pcamv_idr_deblock_launches(int mb_w, int mb_h);
void pcamv_launch_idr_prefix_slices(const IdrJobs &J, int g0, int g, hipStream_t st);
void pcamv_launch_idr_pack_slices(const IdrJobs &J, int g0, int g, int mb_w, int mb_h, hipStream_t st);
void pcamv_launch_idr_unit_len(const IdrJobs &J, int g0, int g, hipStream_t st);
void pcamv_launch_idr_place(const IdrJobs &J, int g0, int g, hipStream_t st);
void pcamv_launch_idr_unit_slices(const IdrJobs &J, int g0, int g, hipStream_t st);
extern "C" int pcamv_gpu_write_idr_slice_header3(const pcamv_stream_params_t *params, int nal_ref_idc, int idr_pic_id, int slice_qp, int deblock, int64_t first_mb,
                                                 uint8_t *bits, size_t cap, int32_t *n_bits)
{
    if (n_bits) *n_bits = 0;
    if (!params || !n_bits || (!bits && cap)) return PCAMV_EINVAL;
    int n = 0;
    TRY(pcamv_idr_header_write3(*params, nal_ref_idc, idr_pic_id, slice_qp, deblock, first_mb, NULL, &n));       /* judged and counted; nothing stored */
    if ((size_t)(n + 7) / 8 > cap) return PCAMV_ENOMEM;
    const int rc = pcamv_idr_header_write3(*params, nal_ref_idc, idr_pic_id, slice_qp, deblock, first_mb, bits, &n);
    *n_bits = n;
    return rc;
}
extern "C" int pcamv_gpu_write_idr_slice_header2(const pcamv_stream_params_t *params, int nal_ref_idc, int idr_pic_id, int slice_qp, int deblock, uint8_t *bits, size_t cap,
                                                 int32_t *n_bits)
{
    return pcamv_gpu_write_idr_slice_header3(params, nal_ref_idc, idr_pic_id, slice_qp, deblock, 0, bits, cap, n_bits);
}
extern "C" int pcamv_gpu_write_idr_slice_header(const pcamv_stream_params_t *params, int nal_ref_idc, int idr_pic_id, int slice_qp, uint8_t *bits, size_t cap, int32_t *n_bits)
{
    return pcamv_gpu_write_idr_slice_header2(params, nal_ref_idc, idr_pic_id, slice_qp, 0, bits, cap, n_bits);
}
extern "C" int64_t pcamv_gpu_idr_bound(const pcamv_ctx_t *c, int as_nal) { return c ? (int64_t)idr_bound(c->F.n_mb, as_nal) : PCAMV_EINVAL; }
extern "C" int64_t pcamv_gpu_idr_bound4(const pcamv_ctx_t *c, int as_nal, int slice_rows, int i4x4)
{
    return c && slice_rows >= 0 && i4x4 >= 0 && i4x4 <= 2 ? (int64_t)idr_bound_slices_bits(c->F.mb_w, c->F.mb_h, slice_rows, as_nal, idr_mb_bits_of(i4x4)) : PCAMV_EINVAL;
}
extern "C" int64_t pcamv_gpu_idr_bound3(const pcamv_ctx_t *c, int as_nal, int slice_rows) { return pcamv_gpu_idr_bound4(c, as_nal, slice_rows, 0); }
/* the working memory of one place of a group: bytes per context.  Per macroblock 24 counts, a slot of 1408, a length of 4, a prefix
 * entry of 8 and 1397.4 of RBSP: 2842; a picture of S > 1 slices adds 64 S per place -- a prefix entry, the room of a header and its
 * paddings in the RBSP (IDR_SLICE_PAD_BYTES), a unit's length and its offset.  A call with i4x4 != 0 adds per macroblock the 16 modes
 * and the 6.4 bytes of RBSP an Intra4x4 macroblock may be longer by (mb_bits: IDR_MB_BITS_I4), and 256 for the modes' own rounding */
static size_t idr_place_bytes(int n_mb, int n_slices, int i4x4, size_t *rbsp_stride)
{
    const size_t S = (size_t)n_slices;
    const int mb_bits = idr_mb_bits_of(i4x4);
    const size_t rbsp = ((size_t)(S > 1 ? idr_slice_rbsp_at_bits(n_mb, n_slices, mb_bits) : idr_bound_bits(n_mb, 0, mb_bits)) + 255) & ~(size_t)255;
    if (rbsp_stride) *rbsp_stride = rbsp;
    return (((size_t)n_mb * (IDR_NZ_BYTES + IDR_SLOT_DWORDS * 4 + 4 + (i4x4 ? IDR_MODE_BYTES : 0)) + ((size_t)n_mb + S) * 8 + (S > 1 ? 16 * S : 0) + rbsp + 255) & ~(size_t)255) +
           (i4x4 ? 512 : 256);          /* (+ 256: the counts of a group end at a multiple of 256; so do the modes) */
}
#define IDR_GROUP_BYTES ((size_t)8 << 30)       /* the most working memory a batch keeps for its IDR pictures: larger batches run in groups */
/* the working memory (made at first use, kept until the batch goes), the tables, and J but for its destination */
static int idr_setup(pcamv_batch *b, int qp, const uint8_t *hdr, int hdr_bits, int nal_byte, int slice_rows, int i4x4, IdrJobs *J)
{
    const pcamv_ctx *c0 = b->ctx[0];
    const int n_mb = c0->F.n_mb, n_slices = idr_n_slices(c0->F.mb_h, slice_rows);
    for (int i = 0; i < b->n; i++) {
        const pcamv_ctx *c = b->ctx[i];
        if (!c->F.fenc[0] || !c->F.fenc[1] || !c->F.fenc[2]) return fail(b, PCAMV_EINVAL, "context %d has no source picture (pcamv_gpu_upload_fenc, pcamv_gpu_set_fenc_device)", i);
        if (c->p.i_luma_deadzone[1] != c0->p.i_luma_deadzone[1]) return fail(b, PCAMV_EINVAL, "the contexts of a batch share one intra dead zone");
    }
    if (c0->p.i_luma_deadzone[1] < 0 || c0->p.i_luma_deadzone[1] > 32) return fail(b, PCAMV_EINVAL, "i_luma_deadzone[1] outside 0 .. 32");
    size_t rbsp_stride = 0;
    const size_t place = idr_place_bytes(n_mb, n_slices, i4x4, &rbsp_stride);
    int group = (int)(IDR_GROUP_BYTES / place);
    group = group < 1 ? 1 : group > b->n ? b->n : group;
    if (!b->d_idr || b->idr_group != group || place * (size_t)group > b->d_idr.cap) {       /* (the last: a call with more slices than any before, or the first with i4x4) */
        if (b->d_idr) HIPCHK(b, hipDeviceSynchronize());    /* (regrown only behind this: pictures in flight work in the block) */
        TRY(b->d_idr.room(b, place * (size_t)group));
        b->idr_group = group;
    }
    if (!b->d_idr_ctx) TRY(b->d_idr_ctx.room(b, (size_t)b->n * (2 * 4 + 3 * 8)));
    if (!b->d_wstat) TRY(b->d_wstat.room(b, (size_t)b->n));
    if (!b->d_idr_tab) {
        uint8_t tab[SV_TAB_BYTES];
        if (sv_build_tables(tab)) return fail(b, PCAMV_EINVAL, "the CAVLC code tables do not fit their entries");
        TRY(b->d_idr_tab.room(b, (size_t)SV_TAB_BYTES));
        HIPCHK(b, hipMemcpy(b->d_idr_tab, tab, SV_TAB_BYTES, hipMemcpyHostToDevice));
    }
    IdrJobs &j = *J;
    memset((void *)&j, 0, sizeof(j));
    const size_t g = (size_t)group, n = (size_t)n_mb;
    uint8_t *at = b->d_idr;
    j.pre = (long long *)at; at += g * (n + (size_t)n_slices) * 8;
    if (n_slices > 1) { j.ulen = (long long *)at; at += g * (size_t)n_slices * 8; j.uoff = (long long *)at; at += g * (size_t)n_slices * 8; }
    j.slots = (uint32_t *)at; at += g * n * IDR_SLOT_DWORDS * 4;
    j.bits = (int *)at; at += g * n * 4;
    j.nz = at; at += (g * n * IDR_NZ_BYTES + 255) & ~(size_t)255;
    if (i4x4) { j.modes = at; at += (g * n * IDR_MODE_BYTES + 255) & ~(size_t)255; }
    j.rbsp = at; j.rbsp_stride = (long long)rbsp_stride;
    j.tab = b->d_idr_tab;
    j.bad = (int *)(b->d_idr_ctx + (size_t)b->n * 24); j.first = j.bad + b->n;
    memcpy(j.hdr, hdr, IDR_HDR_BYTES);
    for (int o = -12; o <= 12; o++) { const int q = qp + o; j.qpc_of[12 + o] = pcamv_chroma_qp_tab[q < 0 ? 0 : q > 51 ? 51 : q]; }
    j.hdr_bits = hdr_bits; j.nal_byte = nal_byte; j.n_mb = n_mb; j.qp = qp; j.dz = c0->p.i_luma_deadzone[1];
    j.status = b->d_wstat;
    j.n_slices = n_slices; j.slice_rows = n_slices > 1 ? slice_rows : 0;
    j.i4x4 = i4x4; j.lambda = pcamv_lambda_tab[qp]; j.mb_bits = idr_mb_bits_of(i4x4);
    return 0;
}
/* the headers of the S > 1 slices of a picture, which differ in first_mb_in_slice alone; the first is the one idr_setup was given */
static int idr_slice_headers(const pcamv_stream_params_t &P, int nal_ref_idc, int idr_pic_id, int qp, int deblock, int mb_w, int mb_h, int slice_rows, std::vector<IdrSliceHdr> *tab)
{
    const int S = idr_n_slices(mb_h, slice_rows);
    tab->assign(S > 1 ? (size_t)S : 0, IdrSliceHdr());
    for (size_t s = 0; s < tab->size(); s++)
        TRY(pcamv_idr_header_write3(P, nal_ref_idc, idr_pic_id, qp, deblock, idr_slice_first_mb(mb_w, mb_h, slice_rows, (int)s), (*tab)[s].hdr, &(*tab)[s].bits));
    return 0;
}
/* every context's source coded, group by group, on `st`; (J.deblock) every picture filtered, all contexts per launch -- k_idr_deblock works
 * on the contexts' reconstruction planes and on nothing of a group's working memory, so it stands behind the groups; then every context's
 * reconstruction becomes its reference: copied into the context's own reference planes, and the plane production of a step with no
 * previous motion -- the state pcamv_gpu_set_ref leaves */
static int idr_run(pcamv_batch *b, IdrJobs &J, const void *sws_ctx, hipStream_t st, const std::vector<IdrSliceHdr> &shdr)
{
    int stage = -1;
    if (J.n_slices > 1) {               /* the S headers: a small table through the staging ring of the writers' headers */
        const size_t total = shdr.size() * sizeof(IdrSliceHdr);
        if ((int)shdr.size() != J.n_slices) return fail(b, PCAMV_EINVAL, "the slices' headers are missing");
        TRY(stage_take(b, b->tx_stage, total, &stage));
        memcpy(b->tx_stage.h[stage], shdr.data(), total);
        TRY(stage_send(b, b->tx_stage, stage, total, st));
        J.shdr = (const IdrSliceHdr *)b->tx_stage.d[stage].p;
        J.units = (SwsCtx *)sws_ctx;
    }
    const FrameDev *dF; const EmbedDev *dE; int slot;
    const int prc = batch_push_descs(b, st, &dF, &dE, &slot);
    if (prc) { if (stage >= 0) stage_release(b, b->tx_stage, stage, st); return prc; }
    J.Fs = dF;
    const FrameDev &F = b->ctx[0]->F;
    if (sws_ctx) pcamv_launch_idr_slot(J, sws_ctx, b->n, st);
    for (int g0 = 0; g0 < b->n; g0 += b->idr_group) {
        const int g = b->n - g0 < b->idr_group ? b->n - g0 : b->idr_group;
        if (J.i4x4) {
            b->kt[KT_IDR_MB4].weight = pcamv_idr_deblock_launches(F.mb_w, F.mb_h);      /* (the anti-diagonals x + 2 y, as the filter's) */
            timed(b, KT_IDR_MB4, st, [&] { pcamv_launch_idr_mb4(J, g0, g, F.mb_w, F.mb_h, st); });
        } else
            timed(b, KT_IDR_MB, st, [&] { pcamv_launch_idr_mb(J, g0, g, F.mb_w, F.mb_h, st); });
        if (J.n_slices > 1) {           /* several slices: a length pass and a placement in front of the units, which a wavefront each then writes */
            timed(b, KT_IDR_PREFIX, st, [&] { pcamv_launch_idr_prefix_slices(J, g0, g, st); });
            timed(b, KT_IDR_PACK, st, [&] { pcamv_launch_idr_pack_slices(J, g0, g, F.mb_w, F.mb_h, st); });
            timed(b, KT_IDR_UNIT_LEN, st, [&] { pcamv_launch_idr_unit_len(J, g0, g, st); });
            timed(b, KT_IDR_PLACE, st, [&] { pcamv_launch_idr_place(J, g0, g, st); });
            timed(b, KT_IDR_UNIT, st, [&] { pcamv_launch_idr_unit_slices(J, g0, g, st); });
            continue;
        }
        timed(b, KT_IDR_PREFIX, st, [&] { pcamv_launch_idr_prefix(J, g0, g, st); });
        timed(b, KT_IDR_PACK, st, [&] { pcamv_launch_idr_pack(J, g0, g, st); });
        timed(b, KT_IDR_UNIT, st, [&] { pcamv_launch_idr_unit(J, g0, g, st); });
    }
    if (stage >= 0) TRY(stage_release(b, b->tx_stage, stage, st));
    if (J.deblock) {
        b->kt[KT_IDR_DEBLOCK].weight = pcamv_idr_deblock_launches(F.mb_w, F.mb_h);      /* one pair of events around the anti-diagonals (all counted, also the empty ones of a picture one macroblock wide) */
        timed(b, KT_IDR_DEBLOCK, st, [&] { pcamv_launch_idr_deblock(J, b->n, F.mb_w, F.mb_h, st); });
    }
    TRY(launched(b));
    TRY(ring_release(b, b->ring, slot, st));
    const size_t ysz = (size_t)F.w * F.h;
    for (int i = 0; i < b->n; i++) {
        pcamv_ctx *c = b->ctx[i];
        for (int k = 0; k < 3; k++) {
            HIPCHK(b, hipMemcpyAsync(c->d_raw[k], c->F.rec[k], k ? ysz / 4 : ysz, hipMemcpyDeviceToDevice, st));
            c->F.raw[k] = c->d_raw[k];
        }
        c->F.have_prev = 0; c->F.ref_is_inter = 0; c->prev_internal = 0;
        c->F.mv = c->d_mv; c->F.ref8 = c->d_ref8; c->F.prev_mv = c->d_prev_mv; c->F.prev_ref = c->d_prev_ref;
        drop_rec_reuse(c);
    }
    return batch_launch(b, ST_PLANES, st);
}
/* the parameter sets the probe's header is written under: pcamv_stream_params_t {4, 0, 4, 0, 0, 0, 1, 0, 0, 26, 1, pps_id} */
static pcamv_stream_params_t idr_probe_params(int pps_id)
{
    pcamv_stream_params_t P = {4, 0, 4, 0, 0, 0, 1, 0, 0, 26, 1, pps_id};
    return P;
}
extern "C" int pcamv_gpu_encode_idr4(pcamv_ctx_t *c, int qp, int pps_id, int idr_pic_id, int as_nal, int deblock, int slice_rows, int i4x4, uint8_t *out, size_t cap, size_t *len)
{
    if (!c || !out || !len || cap > ((size_t)1 << 40)) return PCAMV_EINVAL;
    *len = 0;
    if (slice_rows < 0) return fail(c, PCAMV_EINVAL, "encode_idr3: slice_rows below 0");
    if (i4x4 < 0 || i4x4 > 2) return fail(c, PCAMV_EINVAL, "encode_idr4: i4x4 is 0 (Intra16x16 only), 1 (decided per macroblock) or 2 (Intra4x4 everywhere)");
    if (idr_n_slices(c->F.mb_h, slice_rows) > 1 && !as_nal) return fail(c, PCAMV_EINVAL, "encode_idr3: the RBSPs of several slices behind each other mean nothing: as_nal must be 1");
    HIPCHK(c, hipSetDevice(c->device));
    pcamv_batch *b = c->self;
    TRY(on_behalf(c, b, batch_live(b)));
    uint8_t hdr[IDR_HDR_BYTES] = {0};
    int hdr_bits = 0;
    const pcamv_stream_params_t P = idr_probe_params(pps_id);
    const int hrc = pcamv_idr_header_write2(P, 3, idr_pic_id, qp, deblock, hdr, &hdr_bits);
    if (hrc) return fail(c, hrc, deblock ? "encode_idr2: qp outside 0 .. 51, pps_id outside 0 .. 255, idr_pic_id outside 0 .. 65535 or deblock not 0 or 1"
                                         : "encode_idr: qp outside 0 .. 51, pps_id outside 0 .. 255 or idr_pic_id outside 0 .. 65535");
    std::vector<IdrSliceHdr> shdr;
    TRY(idr_slice_headers(P, 3, idr_pic_id, qp, deblock, c->F.mb_w, c->F.mb_h, slice_rows, &shdr));
    IdrJobs J;
    TRY(on_behalf(c, b, idr_setup(b, qp, hdr, hdr_bits, 3 << 5 | 5, slice_rows, i4x4, &J)));
    DevBuf<uint8_t> d_out;
    TRY(d_out.room(c, cap ? cap : 1));
    long long *arr = (long long *)b->d_idr_ctx.p;
    const long long h_arr[3] = {0, (long long)cap, 0};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(arr, h_arr, sizeof(h_arr), hipMemcpyHostToDevice));
    J.bytes = d_out; J.bytes_size = (long long)cap; J.off = arr; J.cap = arr + 1; J.len = arr + 2; J.as_nal = as_nal != 0; J.first = NULL;
    J.deblock = deblock;
    TRY(on_behalf(c, b, idr_run(b, J, NULL, c->stream, shdr)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int st = 0; long long n = 0;
    HIPCHK(c, hipMemcpy(&st, b->d_wstat, sizeof(st), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&n, arr + 2, sizeof(n), hipMemcpyDeviceToHost));
    if (st) return fail(c, st, st == PCAMV_ENOMEM ? "the IDR unit does not fit %zu bytes (pcamv_gpu_idr_bound gives a capacity that always does)" : "encode_idr: the coder failed", cap);
    if (n < 0 || (size_t)n > cap) return fail(c, PCAMV_EHIP, "encode_idr: length corrupt");
    if (n) HIPCHK(c, hipMemcpy(out, d_out, (size_t)n, hipMemcpyDeviceToHost));
    *len = (size_t)n;
    return 0;
}
extern "C" int pcamv_gpu_encode_idr3(pcamv_ctx_t *c, int qp, int pps_id, int idr_pic_id, int as_nal, int deblock, int slice_rows, uint8_t *out, size_t cap, size_t *len)
{
    return pcamv_gpu_encode_idr4(c, qp, pps_id, idr_pic_id, as_nal, deblock, slice_rows, 0, out, cap, len);
}
extern "C" int pcamv_gpu_encode_idr2(pcamv_ctx_t *c, int qp, int pps_id, int idr_pic_id, int as_nal, int deblock, uint8_t *out, size_t cap, size_t *len)
{
    return pcamv_gpu_encode_idr3(c, qp, pps_id, idr_pic_id, as_nal, deblock, 0, out, cap, len);
}
extern "C" int pcamv_gpu_encode_idr(pcamv_ctx_t *c, int qp, int pps_id, int idr_pic_id, int as_nal, uint8_t *out, size_t cap, size_t *len)
{
    return pcamv_gpu_encode_idr2(c, qp, pps_id, idr_pic_id, as_nal, 0, out, cap, len);
}
extern "C" int pcamv_gpu_batch_write_stream_idr4(pcamv_batch_t *b, int qp, int pps_id, int idr_pic_id, int deblock, int slice_rows, int i4x4, void *stream)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    TRY(batch_live(b));
    if (slice_rows < 0) return fail(b, PCAMV_EINVAL, "write_stream_idr3: slice_rows below 0");
    if (i4x4 < 0 || i4x4 > 2) return fail(b, PCAMV_EINVAL, "write_stream_idr4: i4x4 is 0 (Intra16x16 only), 1 (decided per macroblock) or 2 (Intra4x4 everywhere)");
    StreamOut &O = b->so;
    if (!O.ready) return fail(b, PCAMV_EINVAL, "no byte streams were opened on this batch yet (pcamv_gpu_batch_stream_open)");
    if (O.stepped) return fail(b, PCAMV_EINVAL, "write_stream_idr belongs behind the open and before the first picture of its streams");
    if (O.S.W.first_pic != 0) return fail(b, PCAMV_EINVAL, "an IDR picture is picture 0 of its stream: the open must have first_pic 0");
    pcamv_stream_params_t P = O.S.P;
    P.pps_id = pps_id; P.entropy_cabac = 0;             /* the PPS the IDR slices name: the stream's but for its id and its entropy mode */
    if (!P.deblocking_filter_control_present && deblock != 1)
        return fail(b, PCAMV_EUNSUP, "the IDR picture is not filtered and its header must say so: the PPS needs deblocking_filter_control_present");
    uint8_t hdr[IDR_HDR_BYTES] = {0};
    int hdr_bits = 0;
    const int hrc = pcamv_idr_header_write2(P, O.S.W.nal_ref_idc, idr_pic_id, qp, deblock, hdr, &hdr_bits);
    if (hrc) return fail(b, hrc, deblock ? "write_stream_idr2: qp outside 0 .. 51, pps_id outside 0 .. 255, idr_pic_id outside 0 .. 65535 or deblock not 0 or 1"
                                         : "write_stream_idr: qp outside 0 .. 51, pps_id outside 0 .. 255 or idr_pic_id outside 0 .. 65535");
    hipStream_t st = stream ? (hipStream_t)stream : b->ctx[0]->stream;
    std::vector<IdrSliceHdr> shdr;
    TRY(idr_slice_headers(P, O.S.W.nal_ref_idc, idr_pic_id, qp, deblock, b->ctx[0]->F.mb_w, b->ctx[0]->F.mb_h, slice_rows, &shdr));
    IdrJobs J;
    TRY(idr_setup(b, qp, hdr, hdr_bits, O.S.W.nal_ref_idc << 5 | 5, slice_rows, i4x4, &J));
    const StreamWrite SJ = stream_out_jobs(b);
    J.bytes = SJ.bytes; J.bytes_size = SJ.bytes_size; J.off = SJ.w_off; J.cap = SJ.w_cap; J.len = SJ.w_len; J.first = SJ.first; J.as_nal = 1; J.aud = O.S.W.aud;
    J.deblock = deblock;
    O.stepped = 1;
    TRY(idr_run(b, J, SJ.ctx, st, shdr));
    timed_kernel(b, KT_STREAM_COMMIT, st, k_stream_commit, dim3((b->n + 63) / 64), dim3(64), SJ);
    if (b->rate_open) rate_launch(b, 0, st);
    return launched(b);
}
extern "C" int pcamv_gpu_batch_write_stream_idr3(pcamv_batch_t *b, int qp, int pps_id, int idr_pic_id, int deblock, int slice_rows, void *stream)
{
    return pcamv_gpu_batch_write_stream_idr4(b, qp, pps_id, idr_pic_id, deblock, slice_rows, 0, stream);
}
extern "C" int pcamv_gpu_batch_write_stream_idr2(pcamv_batch_t *b, int qp, int pps_id, int idr_pic_id, int deblock, void *stream)
{
    return pcamv_gpu_batch_write_stream_idr3(b, qp, pps_id, idr_pic_id, deblock, 0, stream);
}
extern "C" int pcamv_gpu_batch_write_stream_idr(pcamv_batch_t *b, int qp, int pps_id, int idr_pic_id, void *stream)
{
    return pcamv_gpu_batch_write_stream_idr2(b, qp, pps_id, idr_pic_id, 0, stream);
}
/* synchronises */
extern "C" int pcamv_gpu_batch_stream_written(pcamv_batch_t *b, int64_t *bytes, int64_t *pictures, int64_t *units)
{
    if (!b) return PCAMV_EINVAL;
    HIPCHK(b, hipSetDevice(b->device));
    if (!b->so.ready) return fail(b, PCAMV_EINVAL, "no byte streams were opened on this batch yet (pcamv_gpu_batch_stream_open)");
    HIPCHK(b, hipDeviceSynchronize());
    HostTmp<SwsCtx> h((size_t)b->n);
    if (!h) return fail(b, PCAMV_ENOMEM, "no memory for %d stream states", b->n);
    HIPCHK(b, hipMemcpy(h.p, b->so.d_own, sizeof(SwsCtx) * (size_t)b->n, hipMemcpyDeviceToHost));
    for (int i = 0; i < b->n; i++) {
        if (bytes) bytes[i] = h.p[i].cur;
        if (pictures) pictures[i] = h.p[i].pic;
        if (units) units[i] = h.p[i].units;
    }
    return 0;
}
/* the parity probe of the header writer: n cases, one lane each */
extern "C" int pcamv_gpu_slice_headers_write_device(pcamv_ctx_t *c, const pcamv_stream_params_t *params, const pcamv_slice_fields_t *fields, int n,
                                                    int32_t *rc_out, int32_t *n_bits, uint8_t *bits)
{
    if (!c || !params || !fields || !rc_out || !n_bits || !bits || n < 1 || n > (1 << 24)) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<pcamv_stream_params_t> d_p; DevBuf<pcamv_slice_fields_t> d_f; DevBuf<int> d_int; DevBuf<uint8_t> d_bits;
    const size_t slots = (size_t)n * PCAMV_SLICE_HDR_BYTES;
    TRY(d_p.room(c, (size_t)n)); TRY(d_f.room(c, (size_t)n)); TRY(d_int.room(c, 2 * (size_t)n)); TRY(d_bits.room(c, slots));
    HIPCHK(c, hipMemcpy(d_p, params, sizeof(*params) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_f, fields, sizeof(*fields) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(d_int, 0xA5, sizeof(int) * 2 * (size_t)n));
    HIPCHK(c, hipMemset(d_bits, 0, slots));
    hipLaunchKernelGGL(k_slice_headers_write, dim3((n + 63) / 64), dim3(64), 0, c->stream, d_p, d_f, n, d_int, d_int + n, d_bits);
    TRY(launched(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(rc_out, d_int, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(n_bits, d_int + n, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(bits, d_bits, slots, hipMemcpyDeviceToHost));
    return 0;
}

/* the time of one of the batch's timed kernels by its name: the launches since the last call, added to the running average */
extern "C" int pcamv_gpu_batch_kernel_time(pcamv_batch_t *b, const char *kernel, double *avg_ms, int *launches, int reset)
{
    if (!b || !kernel) return PCAMV_EINVAL;
    int k = 0;
    while (k < KT_N && strcmp(kernel, kt_name(b, k))) k++;
    if (k == KT_N) return PCAMV_EINVAL;
    KTimer &T = b->kt[k];
    HIPCHK(b, hipSetDevice(b->device));
    HIPCHK(b, hipDeviceSynchronize());
    if (k == KT_ANALYSE) TRY(flow_check(b));
    for (int i = 0; i < T.n; i++) {         /* (a full ring holds the last T.cap launches, in any order: an average does not care) */
        float ms = 0;
        if (hipEventElapsedTime(&ms, T.e0[i], T.e1[i]) == hipSuccess) { T.ms += ms; T.launches += T.weight; }
    }
    T.n = 0; T.head = 0;
    if (avg_ms) *avg_ms = T.launches ? T.ms / T.launches : 0;
    if (launches) *launches = T.launches;
    if (reset) { T.ms = 0; T.launches = 0; }
    return 0;
}
extern "C" int pcamv_gpu_kernel_time(pcamv_ctx_t *c, const char *kernel, double *avg_ms, int *launches, int reset)
{
    if (!c || !kernel || strcmp(kernel, dominant_kernel(c->self))) return PCAMV_EINVAL;
    return pcamv_gpu_batch_kernel_time(c->self, kernel, avg_ms, launches, reset);
}

/* diagnostics: log every block-cost evaluation made for macroblock mb during the next analyse call
 * into a device buffer; fetch with pcamv_gpu_trace_fetch.  mb < 0 switches tracing off. */
extern "C" int pcamv_gpu_trace_mb(pcamv_ctx_t *c, int mb)
{
    if (!c) return PCAMV_EINVAL;
#ifndef PCAMV_TRACE
    if (mb >= 0) return fail(c, PCAMV_EUNSUP, "tracing is compiled out: rebuild with -DPCAMV_TRACE");
#endif
    HIPCHK(c, hipSetDevice(c->device));
    if (mb < 0) { c->F.trace = NULL; return 0; }
    if (!c->d_trace) TRY(ctx_alloc(c, &c->d_trace, (size_t)1 + 8 * 4000));
    HIPCHK(c, hipMemset(c->d_trace, 0, (1 + 8 * 4000) * sizeof(int)));
    c->F.trace = c->d_trace; c->F.trace_mb = mb;
    return 0;
}
extern "C" int pcamv_gpu_trace_fetch(pcamv_ctx_t *c, int32_t *out /* 1 + 8*4000 */)
{
    if (!c || !out || !c->d_trace) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, c->d_trace, (1 + 8 * 4000) * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pcamv_gpu_block_costs(pcamv_ctx_t *c, int qp, int n, const int32_t *req, int32_t *out)
{
    if (!c || !req || !out || n <= 0) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < n; i++) {
        const int32_t *r = req + 8 * i;
        if (r[0] < 0 || r[0] >= c->F.mb_w || r[1] < 0 || r[1] >= c->F.mb_h || r[2] < 0 || r[2] > 6) return fail(c, PCAMV_EINVAL, "request %d", i);
        /* stay inside the 32-pixel padding: the BLOCK (not a 16x16 at its origin) within 24 pixels of the picture, which is as far as the
         * analysis' own MVs take any partition (mv_min / mv_max, pcamv_logic.h); the fetches read one column and two rows more, batch mode
         * one pixel more, and the chroma rows 8 bytes from the block's first sample: all inside the 32 (chroma 16) */
        static const int bw[7] = {16, 16, 8, 8, 8, 4, 4}, bh[7] = {16, 8, 16, 8, 4, 8, 4};
        int px = r[0] * 16 + r[3] + (r[5] >> 2), py = r[1] * 16 + r[4] + (r[6] >> 2);
        if (r[3] < 0 || r[4] < 0 || r[3] + bw[r[2]] > 16 || r[4] + bh[r[2]] > 16) return fail(c, PCAMV_EINVAL, "request %d: block outside its macroblock", i);
        if (px < -28 || py < -28 || px + bw[r[2]] > c->F.w + 24 || py + bh[r[2]] > c->F.h + 24) return fail(c, PCAMV_EINVAL, "request %d leaves the padded plane", i);
    }
    DevBuf<int> d_req, d_out; DevBuf<FrameDev> d_F;
    TRY(probe_frame(c, qp, d_F));
    TRY(d_req.room(c, (size_t)n * 8)); TRY(d_out.room(c, (size_t)n * 3));
    HIPCHK(c, hipMemcpy(d_req, req, (size_t)n * 8 * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_block_costs, dim3(n), dim3(64), 0, c->stream, (const FrameDev *)d_F, (const int *)d_req, (int *)d_out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_out, (size_t)n * 3 * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pcamv_gpu_rd_probe(pcamv_ctx_t *c, int qp, int n, const uint8_t *req, int32_t *out)
{
    if (!c || !req || !out || n <= 0) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<uint8_t> d_req; DevBuf<int> d_out; DevBuf<FrameDev> d_F;
    TRY(probe_frame(c, qp, d_F));
    TRY(d_req.room(c, (size_t)n * 1024)); TRY(d_out.room(c, (size_t)n * 32));
    HIPCHK(c, hipMemcpy(d_req, req, (size_t)n * 1024, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rd_probe, dim3(n), dim3(64), 0, c->stream, (const FrameDev *)d_F, (const uint8_t *)d_req, (int *)d_out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_out, (size_t)n * 32 * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

/* pass-2 substitution (analyse.c:3001-3107) on a fetched record: host-side, trivial */
extern "C" int pcamv_gpu_final_mvs(pcamv_ctx_t *c, pcamv_mb_t *mbs)
{
    if (!c || !mbs) return PCAMV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    int hdr[8];
    HIPCHK(c, hipMemcpy(hdr, c->E.hdr, sizeof(hdr), hipMemcpyDeviceToHost));
    int n = hdr[0];
    if (n < 0 || n > c->cap) return fail(c, PCAMV_EHIP, "embed header corrupt");
    HostTmp<int8_t> flip(n ? n : 1);
    if (!flip) return fail(c, PCAMV_ENOMEM, "flip");
    HIPCHK(c, hipMemcpy(flip, c->d_flip, n, hipMemcpyDeviceToHost));
    int k = 0, slots[16];
    for (int xy = 0; xy < c->F.n_mb; xy++) {
        const int cs = mb_carrier_slots(&mbs[xy], slots);
        for (int i = 0; i < cs && k < n; i++, k++)
            if (flip[k] == 1) { mbs[xy].mv[slots[i]][0] = mbs[xy].mv_stego[slots[i]][0]; mbs[xy].mv[slots[i]][1] = mbs[xy].mv_stego[slots[i]][1]; }
    }
    return 0;
}

/* (sub-matrix columns as the embedder gets them: pcamv_stc_matrix_host, pcamv_stc_extract.h) */
static int host_stc_matrix(int width, int height, unsigned *cols, long long *lcg) { return pcamv_stc_matrix_host(pcamv_stc_mats, width, height, cols, lcg); }
/* syndrome-trellis extractor: H*y over GF(2) with stc_embed's sub-matrix schedule (embed.h:340-393).  lcg: state of the
 * column generator before this frame's embedding (in) / after it (out); NULL = only the tabulated widths */
extern "C" int pcamv_gpu_stc_extract_lcg(const uint8_t *stego, int n, int m, int hgt, int64_t *lcg, uint8_t *message)
{
    if (!stego || !message || n <= 0 || m <= 0 || m > n || hgt < 7 || hgt > 12) return PCAMV_EINVAL;
    double invalpha = (double)n / m;
    int shorter = (int)floor(invalpha), longer = (int)ceil(invalpha);
    unsigned *cs = (unsigned *)malloc(2 * (size_t)STC_MAXW * sizeof(unsigned)), *cl = cs + STC_MAXW;
    if (!cs) return PCAMV_ENOMEM;
    long long st = lcg ? (long long)*lcg : 0;
    /* (host_stc_matrix refuses widths above STC_MAXW.)  The embedder draws the shorter sub-matrix before it finds that the longer one
     * cannot be built (widths 256 / 257), so the generator moves on a frame that fails, too: here as in the embedder and in k_extract_prepare */
    const int built = host_stc_matrix(shorter, hgt, cs, lcg ? &st : NULL) && host_stc_matrix(longer, hgt, cl, lcg ? &st : NULL);
    if (lcg) *lcg = (int64_t)st;
    if (!built) { free(cs); return PCAMV_EUNSUP; }
    memset(message, 0, m);
    int worm = 0, index = 0;
    for (int i = 0; i < m; i++) {
        int lng = worm + longer <= (i + 1) * invalpha + 0.5;
        int width = lng ? longer : shorter;
        const unsigned *cols = lng ? cl : cs;
        worm += width;
        for (int k = 0; k < width && index < n; k++, index++)
            if (stego[index])
                for (int b = 0; b < hgt && i + b < m; b++) message[i + b] ^= (cols[k] >> b) & 1;
    }
    free(cs);
    return 0;
}
extern "C" int pcamv_gpu_stc_extract(const uint8_t *stego, int n, int m, int hgt, uint8_t *message)
{
    return pcamv_gpu_stc_extract_lcg(stego, n, m, hgt, NULL, message);
}
