/*
 * pcamv_variant.h -- what an instance of the analysis kernel has compiled in: the bits of the VARIANT template parameter of the
 * control code (pcamv_logic.h, pcamv_mbkernels.h, pcamv_flow.hip.h).  Plain ints, no HIP type: the device headers read them
 * through pcamv_common.h, the table of RD builds and the CPU test drivers through pcamv_rd_select.h.
 */
#ifndef PCAMV_VARIANT_H
#define PCAMV_VARIANT_H
enum {
    V_TESA = 1,         /* the Hadamard exhaustive search of --me tesa and its run-time choice of the full-pel metric (compiled into the
                         * common instance they cost every other method 11 %) */
    V_RD = 2,           /* the RD mode decision of --subme >= 6 (x264_mb_analyse_p_rd; its code would cost the search of --subme <= 5 registers) */
    V_SPEC = 4,         /* the speculative raster chain (pcamv_flow.hip.h mbk_search_spec) */
    V_RD_PSUB = 8       /* sub-8x8 partitions priced by x264_rd_cost_part: only in builds for one wave per SIMD, which have the registers
                         * for it (compiled into the 4-waves-per-SIMD build it cost 22 spilled VGPRs and 135 more parked scalars) */
};
#endif
