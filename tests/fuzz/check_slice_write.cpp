/* The device slice writer's control code (csrc/pcamv_slice_write.h, what k_write_pslice runs) under AddressSanitizer + UBSan on the
 * CPU: every case writes a slice into a heap block of exactly the capacity the case gives -- the slice's true length, or a few bytes
 * less -- with the writer's working memory in exact-size heap blocks (tests/emu/slice_write_host.h).  A block of the true length
 * must receive the expected bytes; a shorter one must give PCAMV_ENOMEM and length 0.  Built and run by
 * tests/test_slice_write_sanitize.py, which writes the cases (tests/slice_write_cases.py: write_case_file).
 *
 * usage: check_slice_write <cases.bin>     (the case file and what a case must give: check_slice_write_common.h)
 * prints one line per case "<index> <rc> <len> <expected len> <short>" and a summary; exit status 1 on any failure. */
#include "slice_write_host.h"
#include "check_slice_write_common.h"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    return sw_check_cases(argv[1], [](const SliceHostFrame &in, const uint8_t *hdr_bits, int n_bits, int nal_byte, int as_nal, uint8_t *out, long long cap, long long *len) {
        return sw_host_write(in, hdr_bits, n_bits, 0, nal_byte, as_nal, out, cap, len, NULL);
    });
}
