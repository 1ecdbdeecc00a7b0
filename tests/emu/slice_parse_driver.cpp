/*
 * slice_parse_driver.cpp -- TEST-ONLY host build of the CABAC P-slice parser k_parse_pslice runs (csrc/pcamv_slice_parse.h), with
 * scalar primitives.  Lets `pytest -m "not gpu"` compare it record by record with the library's host parser and with slices the
 * reference's own coder wrote.  It is NOT a fallback: libpcamv_gpu.so never links it.
 */
#include "slice_parse_host.h"

extern "C" int spx_parse_at(const uint8_t *rbsp, size_t len, size_t start_bit, int mb_w, int mb_h, int qp, pcamv_mb_t *out)
{
    return sp_host_parse(rbsp, (long long)len, (long long)start_bit, qp, mb_w, mb_h, out);
}
extern "C" int spx_row_bytes(void) { return SP_ROW_BYTES; }
