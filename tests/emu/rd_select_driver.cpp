/*
 * rd_select_driver.cpp -- TEST-ONLY host build of the rules that pick a batch's build of the RD analysis kernel
 * (csrc/pcamv_rd_select.h, what pcamv_gpu_batch_create applies), with the rows of the list of builds the library and the kernel's
 * translation units are made from: name, waves per SIMD, variant of the control code, and the speculative-chain column derived
 * from them.  Lets `pytest -m "not gpu"` pin the selection, and check it against the table, without a GPU.
 */
#include "pcamv_rd_select.h"

#define ROW_NAME(id, occ, variant) #id,
static const char *const names[RD_N_BUILDS] = {PCAMV_RD_BUILDS(ROW_NAME)};
static bool row(int i) { return i >= 0 && i < RD_N_BUILDS; }

extern "C" int rdsel_n_builds(void) { return RD_N_BUILDS; }
extern "C" const char *rdsel_build_name(int i) { return row(i) ? names[i] : ""; }
extern "C" int rdsel_build_spec(int i) { return row(i) ? rd_build_spec(i) : -1; }
extern "C" int rdsel_build_occ(int i) { return row(i) ? rd_build_defs[i].occ : -1; }
extern "C" int rdsel_build_variant(int i) { return row(i) ? rd_build_defs[i].variant : -1; }
extern "C" int rdsel_variant_bit(const char *name)
{
    return !strcmp(name, "V_TESA") ? V_TESA : !strcmp(name, "V_RD") ? V_RD : !strcmp(name, "V_SPEC") ? V_SPEC : !strcmp(name, "V_RD_PSUB") ? V_RD_PSUB : 0;
}
extern "C" int rdsel_spec_min_mbw(void) { return FLOW_SPEC_MIN_MBW; }
extern "C" const char *rdsel_name(int n, int n_cu, int raster, int mb_w, int sub8x8, int tesa, const char *inst, const char *flow_spec)
{
    return rdsel_build_name(rd_select(n, n_cu, raster, mb_w, sub8x8, tesa, inst, flow_spec));
}
