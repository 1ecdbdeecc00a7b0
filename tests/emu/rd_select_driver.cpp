/*
 * rd_select_driver.cpp -- TEST-ONLY host build of the rules that pick a batch's build of the RD analysis kernel
 * (csrc/pcamv_rd_select.h, what pcamv_gpu_batch_create applies), with the names and the speculative-chain column of the list of
 * builds the library makes its table from.  Lets `pytest -m "not gpu"` pin the selection without a GPU.
 */
#include "pcamv_rd_select.h"

#define ROW_NAME(id, sfx, spec) #id,
#define ROW_SPEC(id, sfx, spec) spec,
static const char *const names[RD_N_BUILDS] = {PCAMV_RD_BUILDS(ROW_NAME)};
static const int specs[RD_N_BUILDS] = {PCAMV_RD_BUILDS(ROW_SPEC)};

extern "C" int rdsel_n_builds(void) { return RD_N_BUILDS; }
extern "C" const char *rdsel_build_name(int i) { return i >= 0 && i < RD_N_BUILDS ? names[i] : ""; }
extern "C" int rdsel_build_spec(int i) { return i >= 0 && i < RD_N_BUILDS ? specs[i] : -1; }
extern "C" const char *rdsel_name(int n, int n_cu, int raster, int mb_w, int sub8x8, int tesa, const char *inst, const char *flow_spec)
{
    return rdsel_build_name(rd_select(n, n_cu, raster, mb_w, sub8x8, tesa, inst, flow_spec));
}
