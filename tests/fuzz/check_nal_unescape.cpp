/* The control code of k_nal_to_rbsp (csrc/pcamv_nal_unescape.h) under AddressSanitizer + UBSan on the CPU, with the host form of
 * SP_LANES, against the library's host function pcamv_gpu_nal_to_rbsp (csrc/pcamv_mvsyntax.h) unit by unit: return code, length, bytes
 * and header byte.  Every unit is run with its source in an exact-size heap block at each of the four alignments mod 4 (the block begins
 * 0 .. 3 bytes before the unit and ends with it), its destination in an exact-size heap block of len - 1 bytes at a varying alignment,
 * the working memory in exact-size heap blocks.  The units flagged in the file run once more inside a larger block with other bytes
 * around them (two different surroundings), which must change nothing.  Built and run by tests/test_nal_unescape_cpu.py; the inputs are
 * tests/nal_cases.py's: the ones the GPU test hands to the device afterwards.
 *
 * usage: check_nal_unescape <cases.bin>
 *   cases.bin: int32 {header byte, fill byte, n_fillers}, int32 fillers[]; int32 n_strings, per string uint8 len + bytes -- each string
 *   is wrapped as [start code] header fill^f string, for every filler f and no / the short / the long start code; then int32 n_units,
 *   per unit int32 {twice, len} + bytes
 * prints "units <n> ok <n> err <n> differ <n>"; exit status 1 on any difference. */
#define PCAMV_HOST_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pcamv_host_tables.h"
#include "pcamv_mvsyntax.h"
#include "pcamv_nal_unescape.h"

static long n_units, n_ok, n_err, n_differ;
static NuWork work;             /* the two windows, exact-size heap blocks made once */

/* the control code on unit[0, len) at src, its destination an exact-size block; 1 if it differs from (rc, out[0, n), header) */
static int run_one(const uint8_t *src, size_t len, int dst_align, int rc, const uint8_t *out, size_t n, int header)
{
    const size_t room = len ? len - 1 : 0;
    uint8_t *block = (uint8_t *)malloc(room + dst_align), *dst = block + dst_align;        /* ends where len - 1 bytes end: any write past it is caught */
    memset(block, 0xA5, room + dst_align);
    long long got_n = -7; int got_hdr = -7;
    const int got = pcamv_nal_unescape(work, src, (long long)len, dst, &got_n, &got_hdr);
    int differ = got != rc || got_hdr != header;
    for (int k = 0; k < dst_align; k++) differ |= block[k] != 0xA5;
    if (rc) differ |= got_n != -1;
    else differ |= got_n != (long long)n || (n && memcmp(dst, out, n));
    for (size_t k = rc ? 0 : n; k < room && rc == 0; k++) differ |= dst[k] != 0xA5;        /* nothing behind the RBSP is written either */
    free(block);
    return differ;
}

static void check(const std::vector<uint8_t> &u, int twice)
{
    const size_t len = u.size();
    std::vector<uint8_t> out(len + 1);
    size_t n = 0; int ref_idc = 0, typ = 0;
    const int rc = pcamv_gpu_nal_to_rbsp(u.data(), len, out.data(), &n, &ref_idc, &typ);
    /* the header byte is delivered whatever it is; the host function tells it only of a unit it accepts */
    const size_t at = len >= 4 && !u[0] && !u[1] && !u[2] && u[3] == 1 ? 4 : len >= 3 && !u[0] && !u[1] && u[2] == 1 ? 3 : 0;
    const int header = at < len ? u[at] : -1;
    int differ = rc == 0 && header != (ref_idc << 5 | typ);
    for (int a = 0; a < 4; a++) {
        uint8_t *block = (uint8_t *)malloc(len + a);                /* ends with the unit: any read past it is caught */
        memset(block, 0, a);
        if (len) memcpy(block + a, u.data(), len);
        differ |= run_one(block + a, len, (a + (int)n_units) & 3, rc, out.data(), n, header);
        free(block);
    }
    for (int t = 0; twice && t < 2; t++) {                          /* other bytes around it: nothing outside the unit counts */
        const size_t before = 5 + (size_t)t;
        uint8_t *block = (uint8_t *)malloc(before + len + 8);
        memset(block, t ? 0x00 : 0x03, before + len + 8);
        if (t) { block[before - 1] = 0; block[before + len] = 0xff; block[before + len + 1] = 1; }
        if (len) memcpy(block + before, u.data(), len);
        differ |= run_one(block + before, len, t, rc, out.data(), n, header);
        free(block);
    }
    n_units++;
    if (rc) n_err++; else n_ok++;
    if (differ) { if (n_differ < 20) { printf("differs (host rc %d):", rc); for (size_t k = 0; k < len && k < 24; k++) printf(" %02x", u[k]); printf(" (%zu bytes)\n", len); } n_differ++; }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    work.win = (uint32_t *)malloc(NU_WIN_DWORDS * 4); work.out = (uint32_t *)malloc(NU_OUT_DWORDS * 4);
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[3], count = 0;
    if (fread(h, 4, 3, f) != 3 || h[2] < 0 || h[2] > 64) return 2;
    std::vector<int32_t> fillers(h[2]);
    if (h[2] && fread(fillers.data(), 4, h[2], f) != (size_t)h[2]) return 2;
    static const uint8_t start[3][4] = {{0}, {0, 0, 1}, {0, 0, 0, 1}};
    static const int start_len[3] = {0, 3, 4};
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    for (int k = 0; k < count; k++) {
        uint8_t n, s[255];
        if (fread(&n, 1, 1, f) != 1 || (n && fread(s, 1, n, f) != n)) return 2;
        for (int32_t fl : fillers)
            for (int c = 0; c < 3; c++) {
                std::vector<uint8_t> u(start[c], start[c] + start_len[c]);
                u.push_back((uint8_t)h[0]);
                u.insert(u.end(), (size_t)fl, (uint8_t)h[1]);
                u.insert(u.end(), s, s + n);
                check(u, 0);
            }
    }
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    for (int k = 0; k < count; k++) {
        int32_t g[2];
        if (fread(g, 4, 2, f) != 2 || g[1] < 0) return 2;
        std::vector<uint8_t> u((size_t)g[1]);
        if (g[1] && fread(u.data(), 1, u.size(), f) != u.size()) return 2;
        check(u, g[0]);
    }
    fclose(f);
    free(work.win); free(work.out);
    printf("units %ld ok %ld err %ld differ %ld\n", n_units, n_ok, n_err, n_differ);
    return n_differ ? 1 : 0;
}
