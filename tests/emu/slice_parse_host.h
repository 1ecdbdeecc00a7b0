/*
 * slice_parse_host.h -- TEST-ONLY: the device parser's control code (csrc/pcamv_slice_parse.h) run on the CPU with scalar
 * primitives.  Every piece of the working memory a wave keeps in LDS is a heap block of exactly its size here, so that a sanitizer
 * build reports any index the control code gets wrong.  Used by slice_parse_driver.cpp and tests/fuzz/fuzz_slice_parse.cpp.
 */
#ifndef SLICE_PARSE_HOST_H
#define SLICE_PARSE_HOST_H
#include <stdlib.h>
#include <string.h>
#include "pcamv_entropy_tables.h"
#include "pcamv_slice_parse.h"
#include "slice_host.h"

static inline int sp_host_parse(const uint8_t *rbsp, long long len, long long start_bit, int qp, int mb_w, int mb_h, pcamv_mb_t *out)
{
    if (mb_w < 1 || mb_h < 1) return PCAMV_EINVAL;
    SpState S;
    memset(&S, 0, sizeof(S));
    /* the tables in the block form the device is handed (SP_TAB_*), each in a block of its own */
    int8_t *init_p = (int8_t *)malloc(2 * SP_NCTX);
    uint8_t *trans = (uint8_t *)malloc(256), *rlps = (uint8_t *)malloc(512);
    memcpy(init_p, pcamv_cabac_init_p, 2 * SP_NCTX); memcpy(trans, pcamv_cabac_transition, 256); memcpy(rlps, pcamv_cabac_range_lps, 512);
    const SpTables T = {init_p, trans, rlps};
    S.win = (uint32_t *)calloc(64, 4); S.ctx = (uint8_t *)malloc(SP_NCTX); S.cmvd = (uint32_t *)calloc(48, 4);
    slice_host_alloc(S, (size_t)SP_ROW_BYTES * mb_w, 1);
    const int rc = pcamv_slice_parse(S, T, rbsp, len, start_bit, qp, mb_w, mb_h, out);
    slice_host_free(S);
    free(S.win); free(S.ctx); free(S.cmvd);
    free(init_p); free(trans); free(rlps);
    return rc;
}
#endif
