/* The device CAVLC parser's control code (csrc/pcamv_slice_parse_cavlc.h, what k_parse_pslice_cavlc runs) under AddressSanitizer +
 * UBSan on the CPU, against the library's host parser (mvsyntax::ParserV, csrc/pcamv_mvsyntax.h) input by input: real slices with
 * seeded damage and random bytes in exact-size heap buffers, the parser's working memory in exact-size heap blocks
 * (tests/emu/slice_parse_cavlc_host.h).  The return codes must be equal for every input, and where both are 0 the records.  Built and
 * run by tests/test_slice_parse_cavlc_fuzz.py, which writes the inputs: the same ones the GPU test hands to the device afterwards.
 *
 * usage: fuzz_slice_parse_cavlc <cases.bin>    cases.bin: int32 count, then per case int32 {mb_w, mb_h, qp, start_bit, len} + len bytes
 *                                              (the file form of tests/slice_cases.py; CAVLC reads no QP)
 * prints one line per case "<index> <host rc> <device-code rc>" and a summary; exit status 1 on any difference. */
#define PCAMV_HOST_EMU 1
#include <stdio.h>
#include <vector>
#include "pcamv_host_tables.h"
#include "pcamv_mvsyntax.h"
#include "slice_parse_cavlc_host.h"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    long differ = 0, ok = 0, err = 0;
    for (int k = 0; k < count; k++) {
        int32_t h[5];
        if (fread(h, 4, 5, f) != 5 || h[3] < 0 || h[4] < 0) return 2;
        const int mb_w = h[0], mb_h = h[1];
        const size_t start_bit = (size_t)h[3], len = (size_t)h[4];
        uint8_t *d = (uint8_t *)malloc(len ? len : 1);          /* exact size: any read past the end is caught */
        if (len && fread(d, 1, len, f) != len) return 2;
        std::vector<pcamv_mb_t> a((size_t)mb_w * mb_h), b((size_t)mb_w * mb_h);
        const int ra = pcamv_gpu_parse_pslice_cavlc_at(d, len, start_bit, mb_w, mb_h, a.data());
        const int rb = sv_host_parse(d, (long long)len, (long long)start_bit, mb_w, mb_h, b.data());
        free(d);
        printf("%d %d %d\n", k, ra, rb);
        if (ra != rb) { differ++; continue; }
        if (ra) { err++; continue; }
        ok++;
        if (memcmp(a.data(), b.data(), a.size() * sizeof(pcamv_mb_t))) { printf("%d records differ\n", k); differ++; }
    }
    fclose(f);
    printf("ok %ld err %ld differ %ld\n", ok, err, differ);
    return differ ? 1 : 0;
}
