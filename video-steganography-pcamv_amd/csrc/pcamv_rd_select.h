/*
 * pcamv_rd_select.h -- the builds of the RD instance of the analysis kernel (pcamv_rd*.hip) and which of them a batch runs.
 *
 * Compiles for the host side of the library (pcamv_gpu.hip makes its table of builds from PCAMV_RD_BUILDS and reads the
 * environment) and for a plain C++ test driver (tests/emu/rd_select_driver.cpp): no HIP type.
 */
#ifndef PCAMV_RD_SELECT_H
#define PCAMV_RD_SELECT_H
#include <stdlib.h>
#include <string.h>
#include "pcamv_variant.h"

/* What each build is, stated here only: X(id, waves per SIMD its registers are held to, variant of the control code).  The unit of
 * a build (pcamv_rd*.hip) names its row and compiles the kernel from it, pcamv_gpu.hip makes its table of launchers from the list;
 * PCAMV_RD_INSTANCE names a build by its id */
#define PCAMV_RD_BUILDS(X) \
    X(hi,    4, V_RD) \
    X(lo,    1, V_RD | V_RD_PSUB) \
    X(spec,  1, V_RD | V_SPEC | V_RD_PSUB) \
    X(spec2, 2, V_RD | V_SPEC) \
    X(spec4, 4, V_RD | V_SPEC) \
    X(tesa,  1, V_TESA | V_RD | V_RD_PSUB)
#define PCAMV_RD_ENUM(id, occ, variant) RD_##id,
enum { PCAMV_RD_BUILDS(PCAMV_RD_ENUM) RD_N_BUILDS };
#undef PCAMV_RD_ENUM
struct RdBuildDef { int occ, variant; };
#define PCAMV_RD_DEF(id, occ, variant) {occ, variant},
static constexpr RdBuildDef rd_build_defs[RD_N_BUILDS] = {PCAMV_RD_BUILDS(PCAMV_RD_DEF)};
#undef PCAMV_RD_DEF
/* waves per SIMD of a build's speculative raster chain, 0: plain chain */
static constexpr int rd_build_spec(int build) { return rd_build_defs[build].variant & V_SPEC ? rd_build_defs[build].occ : 0; }
static constexpr bool rd_build_has(int build, int bits) { return (rd_build_defs[build].variant & bits) == bits; }
/* what rd_select (below) takes for granted of the rows it returns */
static_assert(rd_build_has(RD_tesa, V_TESA | V_RD_PSUB) && rd_build_has(RD_spec, V_SPEC | V_RD_PSUB) && rd_build_has(RD_lo, V_RD_PSUB) &&
              !rd_build_spec(RD_tesa) && !rd_build_spec(RD_lo) && !rd_build_spec(RD_hi),
              "rd_select sends --me tesa and sub-8x8 partitions to builds that have them compiled in, and takes tesa, lo and hi for plain chains");

/* chains in a batch up to which the speculative raster schedule is used, and up to which its 1 / 2 waves-per-SIMD builds (measured:
 * below) */
#define PCAMV_SPEC_MAX_CHAINS 3584
#define PCAMV_SPEC1_MAX_CHAINS 320
#define PCAMV_SPEC2_MAX_CHAINS 704
/* narrowest picture, in macroblocks, that takes the speculative chain: a macroblock is handed on once the one FLOW_SPEC_AHEAD
 * (pcamv_flow.hip.h) before it is final, and its top / top-right neighbours, mb_w - 1 .. mb_w + 1 back, must be final by then */
#define FLOW_SPEC_MIN_MBW 8

/* Which build of the RD instance (pcamv_rd.hip) a batch runs: one wave per SIMD while the chains fit that anyway.
 * measured (1080p umh subme 7, MB/s lo / hi): 256 chains 2.31 / 2.21 M, 512: 4.43 / 4.19 M, 1024: 6.84 / 7.77 M -- with one
 * wave per SIMD the lo build has no free wave left at 1024 chains to take the RCA steps off the chains */
/* Five builds (pcamv_rd*.hip).  With CABAC (raster chains) the ones that hand a chain on speculatively after the 16x16
 * search -- ~3 waves work on a chain then --, at 1, 2 or 4 waves per SIMD by the number of chains; measured (1080p umh
 * subme 7, M MB/s, plain / spec1 / spec2 / spec4): 256 chains 2.51 / 4.60 / - / -, 512: 4.81 / 6.77 / 8.17 / 7.90,
 * 1024: 8.40 / 7.31 / 11.9 / 14.0, 2048: 14.3 / 7.30 / 12.5 / 18.3, 3072: 18.4 / - / - / 19.0, 4096: 19.5 / - / - / 19.3.
 * Without a chain (CAVLC: wavefront order) and for thousands of chains the plain builds: "lo" (1 wave per SIMD) while the
 * chains fit that anyway, else "hi" (4).  PCAMV_RD_INSTANCE=lo|hi|spec|spec2|spec4 and PCAMV_FLOW_SPEC=0|1 override.
 * The speculative chain needs pictures >= FLOW_SPEC_MIN_MBW macroblocks wide. */
/* n chains on n_cu compute units; raster: a frame is one chain (FlowDev::raster); sub8x8: sub-8x8 partitions are priced at this level;
 * tesa: a context of the batch searches with --me tesa; inst / flow_spec: PCAMV_RD_INSTANCE / PCAMV_FLOW_SPEC, NULL when unset.
 * Returns the index of the build in PCAMV_RD_BUILDS. */
static inline int rd_select(int n, int n_cu, int raster, int mb_w, int sub8x8, int tesa, const char *inst, const char *flow_spec)
{
    /* --me tesa: its own build (pcamv_rd_tesa.hip), plain chain */
    if (tesa) return RD_tesa;
    const int can_spec = raster && mb_w >= FLOW_SPEC_MIN_MBW;
    const int inst_spec = inst && !strncmp(inst, "spec", 4);
    const int want_spec = inst ? inst_spec : flow_spec ? atoi(flow_spec) != 0 : n <= PCAMV_SPEC_MAX_CHAINS;
    /* sub-8x8 partitions at this level (x264_rd_cost_part, V_RD_PSUB): compiled into the one-wave-per-SIMD builds only */
    if (can_spec && want_spec) {
        if (sub8x8 || (inst && !strcmp(inst, "spec"))) return RD_spec;
        if (inst && !strcmp(inst, "spec2")) return RD_spec2;
        if (inst && !strcmp(inst, "spec4")) return RD_spec4;
        return n <= PCAMV_SPEC1_MAX_CHAINS ? RD_spec : n <= PCAMV_SPEC2_MAX_CHAINS ? RD_spec2 : RD_spec4;
    }
    if (sub8x8) return RD_lo;
    /* a plain build by name; a speculative one that cannot be had, or no name: by the number of chains */
    if (inst && !inst_spec) return !strcmp(inst, "lo") ? RD_lo : RD_hi;
    return raster && n <= 2 * n_cu ? RD_lo : RD_hi;
}
#endif
