/*
 * slice_parse_cavlc_driver.cpp -- TEST-ONLY host build of the CAVLC P-slice parser k_parse_pslice_cavlc runs
 * (csrc/pcamv_slice_parse_cavlc.h), with scalar primitives.  Lets `pytest -m "not gpu"` compare it record by record with the
 * library's host parser and with slices the reference's own coder wrote.  It is NOT a fallback: libpcamv_gpu.so never links it.
 */
#include "slice_parse_cavlc_host.h"

extern "C" int svx_parse_at(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, pcamv_mb_t *out)
{
    if (len > ((size_t)1 << 40) || start_bit > ((size_t)1 << 44)) return PCAMV_EINVAL;
    return sv_host_parse(rbsp, (long long)len, (long long)start_bit, mb_w, mb_h, out);
}
extern "C" int svx_row_bytes(void) { return SV_ROW_BYTES; }
