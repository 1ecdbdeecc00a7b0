/*
 * pcamv_flow.hip.h -- the dataflow schedule of the persistent kernels (gfx950), shared by every unit of the library: the queue
 * descriptor FlowDev, the queue protocol flow_loop<MODE, VARIANT> and the speculative hand-off along a raster chain
 * (mbk_search_spec).  Types, __device__ functions and templates only, never a non-template __global__ function: a kernel is
 * defined in the unit that launches it -- k_analyse_flow and k_pass2_deblock_flow in the main unit (pcamv_kernels.hip.h),
 * k_analyse_flow_tesa in pcamv_tesa.hip, k_analyse_flow_rd in pcamv_rd.hip -- so that no unit compiles, or ships, another's kernels.
 */
#ifndef PCAMV_FLOW_HIP_H
#define PCAMV_FLOW_HIP_H
#include "pcamv_common.h"
#include "pcamv_prims_gpu.h"
#include "pcamv_mbkernels.h"
#include "pcamv_pass2.hip.h"

/* ------------------------------------------------------------------ dataflow scheduling of the analysis
 * One persistent launch per frame step instead of one launch per anti-diagonal: macroblock (x,y) of a
 * GOP becomes ready when (x-1,y) and (x+1,y-1) [or (x,y-1) at the right edge] are done; ready
 * macroblocks of every GOP in flight go through ONE append-only queue.  A wave pops the next index,
 * waits for that entry to be published, runs the search, publishes the motion the neighbours need
 * (agent-scope release), decrements its two successors' dependency counters (the one that reaches 0
 * is appended to the queue), and then -- off the critical path -- does the macroblock's RCA costs and
 * pass-1 reconstruction from the state it just produced.  Nothing depends on dispatch order, on
 * residency or on workgroup->XCD placement: an entry index is only waited for after it was handed out,
 * entries are appended by waves that are running, and the dependency graph always has a ready node
 * until everything is done.  Spins are bounded; a timeout raises ctr[2] and every wave drains. */
struct FlowDev {
    unsigned *ctr;            /* FLOW_HEAD(q) pop index / FLOW_TAIL(q) append index of queue q, FLOW_ERR error flag -- every
                               * counter in a 128-byte line of its own: they are the hottest addresses of the launch, and
                               * with all sixteen in one line every pop and append of the whole chip serialised on it
                               * (23 ns per macroblock: the entire cost of the pass-2 kernel, and a floor under the search) */
    unsigned *queue;          /* total entries, queue x at [qbase[x], qbase[x] + qcount[x]); 0 = not yet published, else (gop << 16 | mb_xy) + 1 */
    int *dep;                 /* [n_gop * n_mb] dependencies still open */
    unsigned total, spin_limit;
    unsigned qbase[8], qcount[8];
    int n_gop, n_mb, mb_w, mb_h, fused, nq;      /* nq = 8: GOP g lives in queue g & 7 (XCD affinity); nq = 1: one queue */
    int unit;                 /* macroblocks of a row per task (second pass only; 1 by default); mb_w / n_mb above are in tasks */
    int raster;               /* --subme >= 6 with CABAC: the slice's context states chain the macroblocks of a frame in raster order
                               * (encoder.c:1900-1927, rdo.c:62), so a macroblock's only predecessor is the one coded before it */
    int spec;                 /* raster chains handed on speculatively (mbk_search_spec below); the launcher picks the kernel instance */
    unsigned *rdone;          /* [n_gop * FLOW_RDONE_STRIDE] per chain: macroblocks of the frame whose FINAL state is published */
};
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define FLOW_HEAD(q) (64 * (q))
#define FLOW_TAIL(q) (64 * (q) + 32)
#define FLOW_ERR 512
#define FLOW_CTR_WORDS 576
#define FLOW_RDONE_STRIDE 32          /* words between two chains' counters: a 128-byte line each */
#define FLOW_SPEC_AHEAD 4             /* a macroblock is handed on only once the one FLOW_SPEC_AHEAD before it is final (so that its top / top-right
                                       * neighbours, mb_w - 1 .. mb_w + 1 back, always are: FLOW_SPEC_MIN_MBW, pcamv_rd_select.h) */

__device__ __forceinline__ unsigned flow_bcast(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ void flow_done_one(const FlowDev &fl, int q, int slot, unsigned item)
{
    if (__hip_atomic_fetch_sub(&fl.dep[slot], 1, RLX_AGENT) == 1) {
        unsigned t = __hip_atomic_fetch_add(&fl.ctr[FLOW_TAIL(q)], 1u, RLX_AGENT);
        __hip_atomic_store(&fl.queue[fl.qbase[q] + t], item, RLX_AGENT);
    }
}

/* ------------------------------------------------------------------ speculative hand-off along a raster chain
 * With CABAC a frame is ONE chain of macroblocks (the context states), and with few GOPs in flight the chip waits for that
 * chain: ~100 us per macroblock, of which the 16x16 search is a third.  What the NEXT macroblock's searches need from this
 * one is its motion only (the left column of its 4x4 motion field, its 16x16 search result, whether it is skipped) -- the
 * entropy coder's state is first read by the RD stage.  And the motion is almost always the 16x16 result (or the skip
 * prediction).  So a macroblock publishes "16x16, this MV" (or its skip) right after its 16x16 search and hands the chain on;
 * its other searches, its RD stage and the successor's searches then run side by side on different waves.  Exact by
 * construction: before its RD stage every macroblock waits until its predecessor is FINAL (rdone), compares the motion it
 * started from with the final one, and starts over if they differ (so does, in turn, whoever started from what it published);
 * what a macroblock commits is computed from verified inputs only.  A macroblock is handed on only once the macroblock
 * FLOW_SPEC_AHEAD before it is final, which keeps the top neighbours (>= mb_w - 1 back) out of the speculation.
 * Waits are on waves that are running and never wait for a younger macroblock: no cycle; all spins are bounded. */
__device__ __forceinline__ bool flow_wait_rdone(const FlowDev &fl, int g, unsigned need)
{
    if (!need) return true;
    const unsigned *p = fl.rdone + FLOW_RDONE_STRIDE * g;
    for (unsigned spins = 0;; spins++) {
        unsigned v = 0;
        if (LANE() == 0) v = __hip_atomic_load(p, RLX_AGENT);
        if (flow_bcast(v) >= need) return true;
        unsigned bad = 0;
        if ((spins & 255u) == 255u) { if (LANE() == 0) bad = __hip_atomic_load(&fl.ctr[FLOW_ERR], RLX_AGENT); bad = flow_bcast(bad); }
        if (bad || spins >= fl.spin_limit) { if (LANE() == 0) __hip_atomic_store(&fl.ctr[FLOW_ERR], 1u, RLX_AGENT); return false; }
        if (spins < 16) __builtin_amdgcn_s_sleep(2); else __builtin_amdgcn_s_sleep(16);
    }
}
/* the left neighbour's motion as this macroblock's searches used it (from the cache and the candidate list: the very values
 * they consumed), and as it is now in memory; equal = the searches stand */
__device__ __forceinline__ bool spec_inputs_final(const FrameDev &F, MBLocal *L)
{
    if (!(L->neighbour & NB_LEFT)) return true;
    const int xy = L->mb_xy, s4 = 4 * F.mb_w, b4 = 4 * (L->mb_y * s4 + L->mb_x);
    const uint32_t m0 = NB_LD32(&FD(F).mv[2 * (b4 - 1)]), m1 = NB_LD32(&FD(F).mv[2 * (b4 - 1 + s4)]);
    const uint32_t m2 = NB_LD32(&FD(F).mv[2 * (b4 - 1 + 2 * s4)]), m3 = NB_LD32(&FD(F).mv[2 * (b4 - 1 + 3 * s4)]);
    const uint32_t r = NB_LD32(&FD(F).mvr[2 * (xy - 1)]);
    const int t = NB_LD8(&FD(F).mb_type[xy - 1]);
    PCAMV_WAVE_SYNC();
    const int16_t (*c)[2] = L->cmv;
    bool ok = m0 == NB_PACK16(c[SCAN8_0 - 1][0], c[SCAN8_0 - 1][1]) && m1 == NB_PACK16(c[SCAN8_0 - 1 + 8][0], c[SCAN8_0 - 1 + 8][1]) &&
              m2 == NB_PACK16(c[SCAN8_0 - 1 + 16][0], c[SCAN8_0 - 1 + 16][1]) && m3 == NB_PACK16(c[SCAN8_0 - 1 + 24][0], c[SCAN8_0 - 1 + 24][1]);
    ok = ok && (t == PCAMV_P_SKIP) == (L->type_left == PCAMV_P_SKIP);
    /* a coded left neighbour's 16x16 result is the first candidate of this macroblock's 16x16 search (predict_mv_ref16x16) */
    if (t != PCAMV_P_SKIP) ok = ok && r == NB_PACK16(L->mvc16[0][0], L->mvc16[0][1]);
    return flow_bcast(ok ? 1u : 0u) != 0u;
}
template <int VARIANT>
__device__ __forceinline__ bool mbk_search_spec(const FrameDev &F, MBLocal *L, Analysis *a, int mb_x, int mb_y, const FlowDev &fl, int g, unsigned item)
{
    const int xy = mb_y * F.mb_w + mb_x, lane = LANE();
    const int s4 = 4 * F.mb_w, s8 = 2 * F.mb_w, b4 = 4 * (mb_y * s4 + mb_x), b8 = 2 * (mb_y * s8 + mb_x);
    bool handed_on = false;
    int skip;
    for (int round = 0;; round++) {
        mb_load(F, L, mb_x, mb_y, false, 0);                 /* neighbours' motion + source pixels; nothing of the entropy coder yet */
        skip = analyse_s16<VARIANT>(F, L, a);
        if (!handed_on) {
            /* what the successor's searches start from: a skipped macroblock's motion is final as it stands (as far as this
             * macroblock's own inputs are), a coded one is announced as 16x16 with the search's result */
            const uint32_t w = skip ? NB_PACK16(L->pskip_mv[0], L->pskip_mv[1]) : NB_PACK16(a->me16x16.mv[0], a->me16x16.mv[1]);
            if (lane < 16) NB_ST32(&FD(F).mv[2 * (b4 + (lane >> 2) * s4 + (lane & 3))], w);
            if (lane == 0) { NB_ST8(&FD(F).mb_type[xy], skip ? PCAMV_P_SKIP : PCAMV_P_L0); NB_ST16(&FD(F).ref8[b8], 0); NB_ST16(&FD(F).ref8[b8 + s8], 0); }
            if (xy + 1 < fl.n_mb) {
                if (!flow_wait_rdone(fl, g, xy + 1 > FLOW_SPEC_AHEAD ? (unsigned)(xy + 1 - FLOW_SPEC_AHEAD) : 0u)) return false;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) flow_done_one(fl, g & (fl.nq - 1), g * fl.n_mb + xy + 1, item + 1u);
            }
            handed_on = true;
        }
        if (!skip) analyse_s_rest<VARIANT>(F, L, a);
        if (!flow_wait_rdone(fl, g, (unsigned)xy)) return false;         /* the macroblock coded before this one is final */
        if (spec_inputs_final(F, L)) break;
        if (round >= 64) { if (lane == 0) __hip_atomic_store(&fl.ctr[FLOW_ERR], 1u, RLX_AGENT); return false; }     /* (cannot happen: the predecessor is final now) */
    }
    /* RD stage: the entropy coder's neighbourhood, the intra borders and the context states as the predecessor left them */
    {
        MbFetch pf;
        prim_mb_fetch(F, mb_x, mb_y, L->neighbour, 1, pf);
        prim_mb_fetch_store(F, L, 1, pf);
    }
    if (!skip) analyse_decide<VARIANT>(F, L, a);
    update_cache(L, a);
    mbk_search_finish<VARIANT>(F, L, a, mb_x, mb_y);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(fl.rdone + FLOW_RDONE_STRIDE * g, (unsigned)(xy + 1), RLX_AGENT);
    return true;
}

#ifndef PCAMV_FLOW_OCC
#define PCAMV_FLOW_OCC 4        /* waves per SIMD the register allocation of the persistent kernel is held to */
#endif
/* the queue protocol, shared by the two persistent kernels; MODE 0: search -> publish -> reconstruction + RCA,
 * MODE 1: pass 2 + loop filter of the macroblock -> publish */
template <int MODE, int VARIANT>
__device__ __forceinline__ void flow_loop(const FrameDev *__restrict__ Fs, const FlowDev &fl, MBLocal &L, Analysis *Ap, P2Unit *Up)
{
    const int lane = LANE();
    /* home queue = this wave's XCD (speed only: the GOPs of one queue are then searched through one L2
     * instead of being replicated in all eight); a wave whose queue is handed out moves on to the others */
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    int home = (int)(xcc & 7u) & (fl.nq - 1), tried = 0;
    /* the queue ticket of the next macroblock is taken before the RCA step of the current one (nothing there depends
     * on other waves), so the atomic's round trip is covered by work instead of being waited for (measured +2 %;
     * reading the queue entry early as well gave nothing more) */
    unsigned ticket = 0;
    bool have_ticket = false;
    PROF_INIT();
    for (;;) {
        const unsigned long long t_pop = PROF_T();
        unsigned idx = ticket;
        if (!have_ticket && lane == 0) idx = __hip_atomic_fetch_add(&fl.ctr[FLOW_HEAD(home)], 1u, RLX_AGENT);
        have_ticket = false;
        idx = flow_bcast(idx);
        if (MODE == 0) PROF_ADD(13, t_pop);
        const unsigned long long t_item = PROF_T();
        if (idx >= fl.qcount[home]) {                      /* this queue is handed out: next one, or done */
            if (++tried >= fl.nq) break;
            home = (home + 1) & (fl.nq - 1);
            continue;
        }
        tried = 0;
        const unsigned slot = fl.qbase[home] + idx;
        unsigned item = 0;
        for (unsigned spins = 0;; spins++) {
            unsigned v = 0;
            if (lane == 0) v = __hip_atomic_load(&fl.queue[slot], RLX_AGENT);
            item = flow_bcast(v);
            if (item) break;
            unsigned bad = 0;
            if ((spins & 255u) == 255u) { if (lane == 0) bad = __hip_atomic_load(&fl.ctr[FLOW_ERR], RLX_AGENT); bad = flow_bcast(bad); }
            if (bad || spins >= fl.spin_limit) break;
            if (spins < 8) __builtin_amdgcn_s_sleep(8); else __builtin_amdgcn_s_sleep(64);
        }
        if (!item) { if (lane == 0) __hip_atomic_store(&fl.ctr[FLOW_ERR], 1u, RLX_AGENT); break; }
        if (MODE == 0) PROF_ADD(14, t_item);
        const unsigned long long t_f = PROF_T();
        /* no agent-scope acquire: the only data of other waves read here is the neighbours' motion, and every such
         * load is itself an agent-scope load (NB_LD*, `sc1`) issued after the queue entry was seen -- so this CU's L1
         * keeps its lines of the reference planes instead of losing them once per macroblock and wave */
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int g = (int)((item - 1u) >> 16), xy = (int)((item - 1u) & 0xffffu);
        const FrameDev F = Fs[g];
        const int y = xy / fl.mb_w, x = xy - y * fl.mb_w;
        if (MODE == 0) PROF_ADD(15, t_f);
        PROF_ADD(MODE ? 13 : 0, t_pop);
        const unsigned long long t_s = PROF_T();
#ifdef PCAMV_SEARCH_CALL
        if (MODE == 0 && lane == 0) L.fdesc = Fs + g;
#endif
        if (MODE == 0 && (VARIANT & V_SPEC)) { if (!mbk_search_spec<VARIANT>(F, &L, Ap, x, y, fl, g, item)) break; }
        else if (MODE == 0) mbk_search<VARIANT>(F, &L, Ap, x, y);
        else {
            const int x0 = fl.unit * x, n = imin(fl.unit, F.mb_w - x0);
            p2_unit_load(F, Up, x0, y, n);
            for (int k = 0; k < n; k++) {
                if (mbk_pass2(F, &L, x0 + k, y, p2_pre(Up, k))) p2_put_mb(Up, &L, k);
                mbk_deblock_unit(F, Up, &L, k, x0 + k, y);
            }
            p2_unit_store(F, Up, x0, y, n);
        }
        PROF_ADD(MODE ? 14 : 1, t_s);
        const unsigned long long t_p = PROF_T();
        /* publish: the motion the neighbours read was stored write-through (NB_ST*, `sc1`); once this wave's stores
         * have drained, the counters / queue entries may follow -- no agent-scope release (it would write back the
         * XCD's whole dirty L2 once per macroblock: measured 13.3 -> 19.9 M MB/s without it) */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (MODE == 0 && (VARIANT & V_SPEC)) { }                    /* the speculative chain hands on inside mbk_search_spec */
        else if (lane == 0 && fl.raster) {
            if (xy + 1 < fl.n_mb) flow_done_one(fl, g & (fl.nq - 1), g * fl.n_mb + xy + 1, item + 1u);
        } else if (lane == 0) {
            const int base = g * fl.n_mb, q = g & (fl.nq - 1);
            if (x + 1 < fl.mb_w) flow_done_one(fl, q, base + xy + 1, item + 1u);
            if (y + 1 < fl.mb_h) {
                if (x >= 1) flow_done_one(fl, q, base + xy + fl.mb_w - 1, item + (unsigned)fl.mb_w - 1u);
                if (x == fl.mb_w - 1) flow_done_one(fl, q, base + xy + fl.mb_w, item + (unsigned)fl.mb_w);
            }
        }
        PROF_ADD(MODE ? 15 : 2, t_p);
        const unsigned long long t_r = PROF_T();
        if (MODE == 0 && fl.fused) {
            /* (not in raster order: a frame is then one chain, its next macroblock is the only work it has, and an entry bound to a
             * ticket whose wave is still busy with this RCA step waits for it while free waves wait for later entries) */
            if (!fl.raster) {
                if (lane == 0) ticket = __hip_atomic_fetch_add(&fl.ctr[FLOW_HEAD(home)], 1u, RLX_AGENT);
                have_ticket = true;
            }
            mbk_rca_encode(F, &L, Ap, xy, 1, (VARIANT & V_RD) && F.b_mbrd);
        }
        PROF_ADD(3, t_r);
        if (MODE == 0) PROF_ADD(4, t_pop);
    }
    PROF_FLUSH();
}

#ifndef PCAMV_PROF                 /* (the counters build keeps its sums and a trial log in LDS as well) */
static_assert(sizeof(MBLocal) + sizeof(Analysis) <= PCAMV_WAVE_LDS_MAX, "the analysis kernels' LDS per wave (MBLocal + Analysis) no longer allows 16 waves per CU");
#endif

/* the macroblock of block blockIdx.x of a launch for the anti-diagonal x + 2y = d (the host's diag_launch sizes the grid); false: none */
__device__ __forceinline__ bool diag_pos(const FrameDev &F, int d, int *x, int *y)
{
    int y_lo = d - (F.mb_w - 1); y_lo = y_lo > 0 ? (y_lo + 1) >> 1 : 0;
    *y = y_lo + (int)blockIdx.x; *x = d - 2 * *y;
    return *y < F.mb_h && *x >= 0 && *x < F.mb_w;
}

/* the second pass and the loop filter one anti-diagonal per launch (PCAMV_SCHED=diag, pcamv_gpu_pass2_pframe) are a unit of their own,
 * pcamv_pass2_diag.hip, so that the unit of k_pass2_deblock_flow holds no other user of the tile's functions; stages: P2D_* */
enum { P2D_PASS2 = 1, P2D_DEBLOCK = 2 };
void pcamv_launch_pass2_diag(int stages, unsigned blocks, unsigned gops, hipStream_t st, const FrameDev *dF, int d);
/* The instances of k_analyse_flow with --me tesa or the RD mode decision of --subme 6 / 7 compiled in are kernels of their own
 * (pcamv_logic.h: the control code is a template on the variant), each in a translation unit of its own, built in parallel with
 * the main one; the library calls them through these launchers.  pcamv_tesa.hip: */
void pcamv_launch_flow_tesa(unsigned waves, hipStream_t st, const FrameDev *dF, const FlowDev &fl);
/* ... and the builds of the RD instance, BUILD = the index of a row of PCAMV_RD_BUILDS (pcamv_rd_select.h): the unit of a build
 * defines the explicit specialisations for its row (pcamv_rd.hip); the phase timers are per translation unit (PCAMV_PROF) */
template <int BUILD> void pcamv_launch_flow_rd(unsigned waves, hipStream_t st, const FrameDev *dF, const FlowDev &fl);
template <int BUILD> int pcamv_flow_rd_waves_per_cu(void);
template <int BUILD> int pcamv_rd_prof_fetch(unsigned long long *out, int reset);
#endif
