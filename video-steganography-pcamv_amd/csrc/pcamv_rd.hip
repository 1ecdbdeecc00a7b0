/*
 * pcamv_rd.hip -- the instance of the analysis kernel with the RD mode decision of --subme 6 / 7 compiled in
 * (x264_mb_analyse_p_rd / x264_rd_cost_mb, encoder/analyse.c:2117-2186, encoder/rdo.c:139-171: intra SATD thresholds, psy-RD,
 * size-only CABAC / CAVLC, context adaptation; pcamv_logic.h "RD mode decision", pcamv_prims_rd_gpu.h).
 *
 * A kernel of its own for the same reason as the --me tesa instance (pcamv_tesa.hip): compiled into the common instance its
 * code costs the search of --subme <= 5 registers (141 spilled VGPRs, 552 bytes of scratch per lane when it was), and in a
 * translation unit of its own so that the library's instances compile side by side.
 *
 * Six builds of it, one translation unit each: this file is the 4-waves-per-SIMD build "hi", and pcamv_rd_lo.hip, pcamv_rd_spec*.hip
 * and pcamv_rd_tesa.hip include it with PCAMV_RD_BUILD naming their row of PCAMV_RD_BUILDS (pcamv_rd_select.h), which says what a
 * build is: the waves per SIMD its registers are held to and the variant of the control code.  The two plain ones differ in the
 * register budget only.  With CABAC a frame is ONE chain of macroblocks (the context states), so a batch of G GOPs keeps G waves busy
 * (+ the RCA work they hand off to whoever is free):
 *   - "lo", 1 wave per SIMD, every register (342 VGPRs in use, lane-derived constants hoisted out of the macroblock loop):
 *     the fastest macroblock.  Used while the chains are few (G <= 2 x CUs): G=64 874 ms per 1080p step, 512: 943 ms = 4.43 M MB/s;
 *   - "hi", 4 waves per SIMD at 128 VGPRs, nothing spilled (the lane number is laundered, pcamv_prims_gpu.h LANE(): with the
 *     lane == k flags hoisted it spilled 149 registers and every reload was a memory round trip in front of its use):
 *     G=1024 7.77 M MB/s (lo: 6.84 M -- no free wave left for the RCA steps), G=4096 19.1 M.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pcamv_rd_select.h"
#ifndef PCAMV_RD_BUILD
#define PCAMV_RD_BUILD hi
#endif
#define RD_ID_(id) RD_##id
#define RD_ID(id) RD_ID_(id)
static constexpr int RD_BUILD = RD_ID(PCAMV_RD_BUILD);         /* this unit's row of PCAMV_RD_BUILDS */
#ifdef PCAMV_RD_OCC                 /* development: the registers of the hi build re-budgeted for an experiment (tools/dbg/build_fast.sh, EXTRA=-DPCAMV_RD_OCC=n) */
static constexpr int RD_OCC = RD_BUILD == RD_hi ? PCAMV_RD_OCC : rd_build_defs[RD_BUILD].occ;
#else
static constexpr int RD_OCC = rd_build_defs[RD_BUILD].occ;
#endif
static constexpr int RD_VARIANT = rd_build_defs[RD_BUILD].variant;
/* pcamv_prims_gpu.h LANE(): a build for one wave per SIMD has the registers to keep what is computed from the lane number */
static constexpr bool RD_ONE_WAVE = rd_build_defs[RD_BUILD].occ == 1;
#define PCAMV_RD_LO RD_ONE_WAVE
#define PCAMV_SATD_MAT (!(RD_VARIANT & V_TESA))       /* pcamv_prims_gpu.h: the --me tesa build keeps the packed SATD for its 16x16 lists */
#define PCAMV_RESIDUAL_CALL 1      /* pcamv_prims_rd_gpu.h: the CABAC residual walk as a function of its own */
#include "pcamv_flow.hip.h"

static __global__ void __launch_bounds__(64, RD_OCC) k_analyse_flow_rd(const FrameDev *__restrict__ Fs, FlowDev fl)
{
    __shared__ MBLocal L;
    __shared__ Analysis A;
    flow_loop<0, RD_VARIANT>(Fs, fl, L, &A, nullptr);
}

template <> void pcamv_launch_flow_rd<RD_BUILD>(unsigned waves, hipStream_t st, const FrameDev *dF, const FlowDev &fl)
{
    hipLaunchKernelGGL(k_analyse_flow_rd, dim3(waves), dim3(64), 0, st, dF, fl);
}
template <> int pcamv_flow_rd_waves_per_cu<RD_BUILD>(void)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_analyse_flow_rd, 64, 0) != hipSuccess) return -1;
    return per_cu;
}
#ifdef PCAMV_PROF
/* the phase timers are per translation unit (static __device__): this instance's */
template <> int pcamv_rd_prof_fetch<RD_BUILD>(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pcamv_prof), sizeof(unsigned long long) * PCAMV_PROF_N) != hipSuccess) return -1;
    if (reset) { unsigned long long z[PCAMV_PROF_N] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(pcamv_prof), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif
