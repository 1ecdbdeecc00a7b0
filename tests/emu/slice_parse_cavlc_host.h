/*
 * slice_parse_cavlc_host.h -- TEST-ONLY: the device CAVLC parser's control code (csrc/pcamv_slice_parse_cavlc.h) run on the CPU with
 * scalar primitives.  Every piece of the working memory a wave keeps in LDS is a heap block of exactly its size here, so that a
 * sanitizer build reports any index the control code gets wrong.  Used by slice_parse_cavlc_driver.cpp and
 * tests/fuzz/fuzz_slice_parse_cavlc.cpp.
 */
#ifndef SLICE_PARSE_CAVLC_HOST_H
#define SLICE_PARSE_CAVLC_HOST_H
#include <stdlib.h>
#include <string.h>
#include "pcamv_slice_parse_cavlc.h"
#include "slice_host.h"

static inline int sv_host_parse(const uint8_t *rbsp, long long len, long long start_bit, int mb_w, int mb_h, pcamv_mb_t *out)
{
    if (mb_w < 1 || mb_h < 1) return PCAMV_EINVAL;
    SvState S;
    memset((void *)&S, 0, sizeof(S));
    /* the tables in the block form the device is handed (SV_T_*), the two parts in a block each */
    uint8_t tab[SV_TAB_BYTES];
    if (sv_build_tables(tab)) return -100;                /* a table entry that does not fit: never a parser's code */
    uint16_t *vlc = (uint16_t *)malloc(2 * SV_T_N);
    uint8_t *cbp_of = (uint8_t *)malloc(48);
    memcpy(vlc, tab, 2 * SV_T_N); memcpy(cbp_of, tab + SV_T_CBP, 48);
    S.vlc = vlc; S.cbp_of = cbp_of;
    S.win = (uint32_t *)calloc(64, 4);
    slice_host_alloc(S, (size_t)SV_ROW_BYTES * mb_w, 1);
    const int rc = pcamv_slice_parse_cavlc(S, rbsp, len, start_bit, mb_w, mb_h, out);
    slice_host_free(S);
    free(S.win);
    free(vlc); free(cbp_of);
    return rc;
}
#endif
