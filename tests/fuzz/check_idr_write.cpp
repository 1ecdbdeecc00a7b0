/* The device IDR coder's control code (csrc/pcamv_idr.h, what k_idr_mb, k_idr_pack and k_idr_unit run) on the CPU in the scalar form of
 * SP_LANES, under AddressSanitizer + UBSan when tests/test_idr_cpu.py builds it: every case's picture is coded macroblock by macroblock
 * in anti-diagonal order, its RBSP merged dword by dword, its unit written into a heap block of exactly its length, and the RBSP decoded
 * by the library's independent host decoder pcamv_gpu_decode_islice_cavlc (csrc/pcamv_mvsyntax.h).  Every piece of working memory is a
 * heap block of exactly its size.  Required per case: the decoded planes equal the coder's own reconstruction byte for byte; the
 * macroblocks' bit counts and the header's add up to the prefix's total and to the RBSP's length; no level went past the clamp (the
 * writer's own clip never fired); a block one byte short gives PCAMV_ENOMEM.  Then the decoder is fed damaged and truncated slices.
 *
 * usage: check_idr_write <cases.bin> <out.bin> <fuzz iterations per case> [<streams.bin>]      (the case file: tests/idr_cases.py write_case_file)
 * prints one line per case "<index> <rc> <unit bytes> <rbsp bytes> <levels clamped> <00 00 0x in the RBSP> <mode of macroblock (1,1) or -1>"
 * and a summary "cases <n> bad <n> clamped <n> emulation <n>"; out.bin receives per case int64 length + the unit, then the coder's
 * reconstruction.  Exit status 1 on any failure, 2 for a file that is no case file.
 *
 * streams.bin (tests/test_idr_cpu.py writes it from tests/golden/islice_ref_*.npz): I slices another coder made, with the planes that coder
 * reconstructed -- int32 count, then per stream int32 mb_w, mb_h, qp, chroma offset, start bit, bytes; the bytes; Y, U, V.  Each is decoded
 * from a heap block of exactly its size and must give those planes: "ref <index> <rc> <planes equal>" per stream and "refs <n> bad <n>",
 * printed before the cases' lines. */
#include "slice_write_cavlc_host.h"
#include "pcamv_idr.h"
#include "pcamv_mvsyntax.h"
#include <stdio.h>
#include <random>
#include <vector>

struct Case { int32_t mb_w, mb_h, qp, dz, qpc, chroma_offset, hdr_bits, nal_byte; uint8_t hdr[IDR_HDR_BYTES]; std::vector<uint8_t> pl[3]; };

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!f || !fo) return 2;
    const int iters = atoi(argv[3]);
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    uint8_t *tab = (uint8_t *)malloc(SV_TAB_BYTES);
    if (sv_build_tables(tab)) return 2;
    std::mt19937 rng(11);
    long bad = 0, ref_bad = 0, clamped_cases = 0, emul_cases = 0;
    if (argc > 4) {
        FILE *fr = fopen(argv[4], "rb");
        int32_t n = 0;
        if (!fr || fread(&n, 4, 1, fr) != 1 || n < 0) return 2;
        for (int k = 0; k < n; k++) {
            int32_t h[6];
            if (fread(h, 4, 6, fr) != 6 || h[0] < 1 || h[1] < 1 || h[0] * h[1] > 4096 || h[4] < 0 || h[5] < 1 || h[5] > (1 << 24)) return 2;
            const size_t ysz = (size_t)256 * h[0] * h[1];
            std::vector<uint8_t> data((size_t)h[5]), want[3] = {std::vector<uint8_t>(ysz), std::vector<uint8_t>(ysz / 4), std::vector<uint8_t>(ysz / 4)};
            if (fread(data.data(), 1, data.size(), fr) != data.size()) return 2;
            for (auto &w : want) if (fread(w.data(), 1, w.size(), fr) != w.size()) return 2;
            std::vector<uint8_t> dy(ysz), du(ysz / 4), dv(ysz / 4);
            const int rc = pcamv_gpu_decode_islice_cavlc(data.data(), data.size(), (size_t)h[4], h[0], h[1], h[2], h[3], dy.data(), du.data(), dv.data());
            const int same = !rc && dy == want[0] && du == want[1] && dv == want[2];
            printf("ref %d %d %d\n", k, rc, same);
            ref_bad += !same;
        }
        fclose(fr);
        printf("refs %d bad %ld\n", (int)n, ref_bad);
    }
    for (int k = 0; k < count; k++) {
        Case c;
        if (fread(&c.mb_w, 4, 8, f) != 8 || fread(c.hdr, 1, IDR_HDR_BYTES, f) != IDR_HDR_BYTES) return 2;
        if (c.mb_w < 1 || c.mb_h < 1 || c.mb_w * c.mb_h > 4096 || c.hdr_bits < 0 || c.hdr_bits > IDR_HDR_MAX_BITS) return 2;
        const int n_mb = c.mb_w * c.mb_h;
        const size_t ysz = (size_t)256 * n_mb;
        for (int i = 0; i < 3; i++) { c.pl[i].resize(i ? ysz / 4 : ysz); if (fread(c.pl[i].data(), 1, c.pl[i].size(), f) != c.pl[i].size()) return 2; }
        /* working memory, exact sizes */
        uint8_t *rec[3] = {(uint8_t *)malloc(ysz), (uint8_t *)malloc(ysz / 4), (uint8_t *)malloc(ysz / 4)};
        uint8_t *nz = (uint8_t *)malloc((size_t)IDR_NZ_BYTES * n_mb);
        uint32_t *slots = (uint32_t *)malloc((size_t)IDR_SLOT_DWORDS * 4 * n_mb);
        int *bits = (int *)malloc(sizeof(int) * n_mb), *clamped = (int *)malloc(sizeof(int) * n_mb);
        long long *pre = (long long *)malloc(sizeof(long long) * (n_mb + 1));
        IdrWork *W = (IdrWork *)malloc(sizeof(IdrWork));
        memset(rec[0], 0xA5, ysz); memset(rec[1], 0xA5, ysz / 4); memset(rec[2], 0xA5, ysz / 4);
        IdrPic P = {{c.pl[0].data(), c.pl[1].data(), c.pl[2].data()}, {rec[0], rec[1], rec[2]}, c.mb_w, c.mb_h, c.qp, c.qpc, c.dz, nz, slots, bits, clamped};
        for (int d = 0; d < c.mb_w + c.mb_h - 1; d++)
            for (int my = 0; my < c.mb_h; my++) { const int mx = d - my; if (mx >= 0 && mx < c.mb_w) idr_mb(*W, P, (const uint16_t *)tab, mx, my); }
        int ok = 1, n_clamped = 0;
        long long at = c.hdr_bits;
        for (int i = 0; i < n_mb; i++) { pre[i] = at; if (bits[i] < 0) ok = 0; else at += bits[i]; n_clamped += clamped[i]; }
        pre[n_mb] = at;
        const long long rbsp_len = idr_rbsp_bytes(at), dwords = (rbsp_len + 3) / 4;
        uint8_t *rbsp = (uint8_t *)aligned_alloc(4, (size_t)dwords * 4);
        for (long long q = 0; q < dwords; q++) { const uint32_t v = idr_pack_dword(q, c.hdr, c.hdr_bits, pre, slots, n_mb); memcpy(rbsp + 4 * q, &v, 4); }
        for (long long q = rbsp_len; q < dwords * 4; q++) if (rbsp[q]) ok = 0;                /* nothing behind the trailing bits */
        if (!(rbsp[rbsp_len - 1] & 0xff) || (at + 1 + 7) / 8 != rbsp_len) ok = 0;           /* the stop bit is in the last byte */
        int emul = 0;
        for (long long q = 0; q + 2 < rbsp_len; q++) emul |= rbsp[q] == 0 && rbsp[q + 1] == 0 && rbsp[q + 2] <= 3;
        /* the unit: first counted with no room at all, then into a block of exactly its length, then one byte short */
        IdrOut O; uint32_t *win = (uint32_t *)malloc(256); O.obuf = (uint32_t *)malloc(SW_OBUF);
        long long len = -1, want = 0;
        { want = 5; int zeros = 0; for (long long q = 0; q < rbsp_len; q++) { if (zeros == 2 && rbsp[q] <= 3) { want++; zeros = 0; } zeros = rbsp[q] == 0 ? zeros + 1 : 0; want++; } }
        uint8_t *unit = (uint8_t *)malloc((size_t)want);
        int rc = idr_unit(O, win, rbsp, rbsp_len, c.nal_byte, 1, unit, want, &len);
        if (rc || len != want) ok = 0;
        { uint8_t *less = (uint8_t *)malloc((size_t)want - 1); long long l2 = -1; if (idr_unit(O, win, rbsp, rbsp_len, c.nal_byte, 1, less, want - 1, &l2) != PCAMV_ENOMEM || l2 != 0) ok = 0; free(less); }
        if (want > idr_bound(n_mb, 1)) ok = 0;
        /* the unit, unescaped by hand, is the RBSP */
        {
            std::vector<uint8_t> back;
            int zeros = 0;
            for (long long q = 5; q < want; q++) { if (zeros == 2 && unit[q] == 3) { zeros = 0; continue; } zeros = unit[q] == 0 ? zeros + 1 : 0; back.push_back(unit[q]); }
            if (want < 5 || unit[0] || unit[1] || unit[2] || unit[3] != 1 || unit[4] != c.nal_byte || (long long)back.size() != rbsp_len || memcmp(back.data(), rbsp, (size_t)rbsp_len)) ok = 0;
        }
        /* the independent decoder, from an exact-size copy of the RBSP */
        std::vector<uint8_t> exact(rbsp, rbsp + rbsp_len);
        std::vector<uint8_t> dy(ysz), du(ysz / 4), dv(ysz / 4);
        const int drc = pcamv_gpu_decode_islice_cavlc(exact.data(), exact.size(), (size_t)c.hdr_bits, c.mb_w, c.mb_h, c.qp, c.chroma_offset, dy.data(), du.data(), dv.data());
        if (drc || memcmp(dy.data(), rec[0], ysz) || memcmp(du.data(), rec[1], ysz / 4) || memcmp(dv.data(), rec[2], ysz / 4)) ok = 0;
        int mode = -1;                                  /* Intra16x16PredMode of the interior macroblock (1, 1): (mb_type - 1) & 3, mb_type the slot's first ue */
        if (c.mb_w >= 3 && c.mb_h >= 3) {
            const unsigned v = slots[(size_t)IDR_SLOT_DWORDS * (c.mb_w + 1)] >> 16;
            const int z = __builtin_clz(v | 1u) - 16;
            mode = (int)((((v >> (15 - 2 * z)) - 1u) - 1u) & 3u);
        }
        printf("%d %d %lld %lld %d %d %d\n", k, ok ? 0 : drc ? drc : -100, want, rbsp_len, n_clamped, emul, mode);
        bad += !ok; clamped_cases += n_clamped != 0; emul_cases += emul;
        fwrite(&want, 8, 1, fo); fwrite(unit, 1, (size_t)want, fo);
        fwrite(rec[0], 1, ysz, fo); fwrite(rec[1], 1, ysz / 4, fo); fwrite(rec[2], 1, ysz / 4, fo);
        /* the decoder on damaged, truncated and random bytes, each in a block of exactly its size: any code, no report */
        for (int it = 0; it < iters; it++) {
            std::vector<uint8_t> dmg = exact;
            const int nflip = 1 + rng() % 6;
            for (int i = 0; i < nflip; i++) dmg[rng() % dmg.size()] ^= (uint8_t)(1 + rng() % 255);
            if (it % 3 == 0) dmg.resize(1 + rng() % dmg.size());
            if (it % 5 == 0) for (auto &b : dmg) b = (uint8_t)rng();
            const size_t sb = it % 7 == 0 ? rng() % (dmg.size() * 8) : (size_t)c.hdr_bits;
            (void)pcamv_gpu_decode_islice_cavlc(dmg.data(), dmg.size(), sb, c.mb_w, c.mb_h, c.qp, c.chroma_offset, dy.data(), du.data(), dv.data());
        }
        free(unit); free(win); free(O.obuf); free(rbsp); free(W); free(pre); free(bits); free(clamped); free(slots); free(nz);
        for (int i = 0; i < 3; i++) free(rec[i]);
    }
    fclose(f); fclose(fo);
    free(tab);
    printf("cases %d bad %ld clamped %ld emulation %ld\n", count, bad, clamped_cases, emul_cases);
    return bad || ref_bad ? 1 : 0;
}
