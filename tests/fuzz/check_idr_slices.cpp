/* IDR pictures of several slices: the device coder's control code (csrc/pcamv_idr.h, pcamv_idr_defs.h -- what k_idr_mb, k_idr_prefix_slices,
 * k_idr_pack_slices, k_idr_unit_len, k_idr_place and k_idr_unit_slices run) on the CPU in the scalar form of SP_LANES, under
 * AddressSanitizer + UBSan when tests/test_idr_slices_cpu.py builds it.  Per case the picture is coded macroblock by macroblock in
 * anti-diagonal order with IdrPic::slice_rows set, the prefix restarted per slice (idr_prefix_slices), every slice's RBSP merged dword by
 * dword at its place in the RBSP area (whose bytes between the slices must stay untouched), every unit's length counted by the writer's
 * walk (idr_unit_walk, count) and checked against a count by hand, the units placed (idr_place) and written into ONE heap block of exactly
 * the picture's total length -- once in reverse order, once odd slices first -- with every byte outside the unit just written compared
 * after each unit.  Required per case:
 *   (a) pcamv_gpu_decode_idr_picture of the bytes gives the coder's own reconstruction (of a filtered picture: that reconstruction through
 *       pcamv_gpu_deblock_intra_picture);
 *   (b) every slice's RBSP is byte for byte what the one-slice path (slice_rows 0: idr_mb, the serial prefix of check_idr_write.cpp,
 *       idr_pack_dword) makes under the same header for a picture that consists of the slice's source rows, and the reconstruction of that
 *       picture is the slice's rows;
 *   (c) the length pass equals the written length; a capacity of one byte less is PCAMV_ENOMEM and no byte is stored;
 *   (d) (by the test, on this program's output) slice_rows 0 and slice_rows >= mb_h give check_idr_write's bytes.
 *
 * usage: check_idr_slices <cases.bin> <out.bin>        (the case file: tests/idr_slice_cases.py write_case_file)
 * prints per case "<index> <rc> <total bytes> <slices> <a non-first slice holds 00 00 0x> <mask of (first byte of a non-first unit) mod 4>"
 * and "cases <n> bad <n>"; out.bin receives per case int64 length + the units, then the coder's unfiltered reconstruction.  The headers are
 * pcamv_idr_header_write3's under the parameter sets of Encoder.encode_idr with pps_id 1 and nal_ref_idc 3.  Exit status 1 on any failure,
 * 2 for a file that is no case file. */
#include "slice_write_cavlc_host.h"
#include "pcamv_idr.h"
#include "pcamv_mvsyntax.h"
#include <stdio.h>
#include <vector>

struct Case { int32_t mb_w, mb_h, qp, dz, qpc, chroma_offset, slice_rows, idr_pic_id, deblock; std::vector<uint8_t> pl[3]; };

/* a picture (or the rows of one) coded in anti-diagonal order; the working memory is heap blocks of exactly their sizes */
struct Coded {
    uint8_t *rec[3], *nz; uint32_t *slots; int *bits, *clamped; int n_mb;
    Coded(int mb_w, int mb_h) : n_mb(mb_w * mb_h)
    {
        const size_t ysz = (size_t)256 * n_mb;
        rec[0] = (uint8_t *)malloc(ysz); rec[1] = (uint8_t *)malloc(ysz / 4); rec[2] = (uint8_t *)malloc(ysz / 4);
        memset(rec[0], 0xA5, ysz); memset(rec[1], 0xA5, ysz / 4); memset(rec[2], 0xA5, ysz / 4);
        nz = (uint8_t *)malloc((size_t)IDR_NZ_BYTES * n_mb); slots = (uint32_t *)malloc((size_t)IDR_SLOT_DWORDS * 4 * n_mb);
        bits = (int *)malloc(sizeof(int) * n_mb); clamped = (int *)malloc(sizeof(int) * n_mb);
    }
    ~Coded() { for (auto *p : rec) free(p); free(nz); free(slots); free(bits); free(clamped); }
    IdrPic run(const uint8_t *const src[3], int mb_w, int mb_h, const Case &c, int slice_rows, IdrWork *W, const uint8_t *tab)
    {
        IdrPic P = {{src[0], src[1], src[2]}, {rec[0], rec[1], rec[2]}, mb_w, mb_h, c.qp, c.qpc, c.dz, nz, slots, bits, clamped, slice_rows};
        for (int d = 0; d < mb_w + mb_h - 1; d++)
            for (int my = 0; my < mb_h; my++) { const int mx = d - my; if (mx >= 0 && mx < mb_w) idr_mb(*W, P, (const uint16_t *)tab, mx, my); }
        return P;
    }
};

/* an RBSP's unit counted by hand: start code, header byte, a 03 behind every 00 00 in front of a byte <= 3 */
static long long unit_bytes(const uint8_t *rbsp, long long len)
{
    long long want = 5; int zeros = 0;
    for (long long q = 0; q < len; q++) { if (zeros == 2 && rbsp[q] <= 3) { want++; zeros = 0; } zeros = rbsp[q] == 0 ? zeros + 1 : 0; want++; }
    return want;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!f || !fo) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    uint8_t *tab = (uint8_t *)malloc(SV_TAB_BYTES);
    if (sv_build_tables(tab)) return 2;
    const pcamv_stream_params_t probe = {4, 0, 4, 0, 0, 0, 1, 0, 0, 26, 1, 1};
    const int nal_byte = 0x65;
    long bad = 0;
    for (int k = 0; k < count; k++) {
        Case c;
        if (fread(&c.mb_w, 4, 9, f) != 9) return 2;
        if (c.mb_w < 1 || c.mb_h < 1 || c.mb_w * c.mb_h > 4096 || c.slice_rows < 0) return 2;
        const int n_mb = c.mb_w * c.mb_h, S = idr_n_slices(c.mb_h, c.slice_rows);
        const size_t ysz = (size_t)256 * n_mb, lw = (size_t)16 * c.mb_w, cw = (size_t)8 * c.mb_w;
        for (int i = 0; i < 3; i++) { c.pl[i].resize(i ? ysz / 4 : ysz); if (fread(c.pl[i].data(), 1, c.pl[i].size(), f) != c.pl[i].size()) return 2; }
        int ok = 1;
        IdrWork *W = (IdrWork *)malloc(sizeof(IdrWork));
        const uint8_t *const src[3] = {c.pl[0].data(), c.pl[1].data(), c.pl[2].data()};
        Coded pic(c.mb_w, c.mb_h);
        const IdrPic P = pic.run(src, c.mb_w, c.mb_h, c, c.slice_rows, W, tab);
        /* the headers, the prefix, every slice's RBSP at its place */
        IdrSliceHdr *shdr = (IdrSliceHdr *)calloc((size_t)S, sizeof(IdrSliceHdr));
        for (int s = 0; s < S; s++)
            if (pcamv_idr_header_write3(probe, 3, c.idr_pic_id, c.qp, c.deblock, idr_slice_first_mb(c.mb_w, c.mb_h, c.slice_rows, s), shdr[s].hdr, &shdr[s].bits) ||
                shdr[s].bits > IDR_HDR_MAX_BITS) ok = 0;
        long long *pre = (long long *)malloc(sizeof(long long) * (size_t)(n_mb + S));
        if (idr_prefix_slices(P, shdr, pre)) ok = 0;
        const long long area = idr_slice_rbsp_at(n_mb, S);
        uint8_t *rbsp = (uint8_t *)aligned_alloc(4, (size_t)area);
        memset(rbsp, 0xA5, (size_t)area);
        long long *ulen = (long long *)malloc(sizeof(long long) * (size_t)S), *uoff = (long long *)malloc(sizeof(long long) * (size_t)S);
        IdrOut O; uint32_t *win = (uint32_t *)malloc(256); O.obuf = (uint32_t *)malloc(SW_OBUF);
        int emul_later = 0;
        std::vector<long long> at(S), rlen(S);
        for (int s = 0; s < S; s++) {
            const int fm = idr_slice_first_mb(c.mb_w, c.mb_h, c.slice_rows, s), n = idr_slice_n_mb(c.mb_w, c.mb_h, c.slice_rows, s);
            const long long *q = pre + idr_slice_pre_at(fm, s);
            at[s] = idr_slice_rbsp_at(fm, s); rlen[s] = idr_rbsp_bytes(q[n]);
            const long long dwords = (rlen[s] + 3) / 4, next = idr_slice_rbsp_at(fm + n, s + 1);
            if (at[s] + 4 * dwords > next || next > area) { ok = 0; continue; }
            for (long long d = 0; d < dwords; d++) { const uint32_t v = idr_pack_dword(d, shdr[s].hdr, shdr[s].bits, q, pic.slots + (size_t)fm * IDR_SLOT_DWORDS, n); memcpy(rbsp + at[s] + 4 * d, &v, 4); }
            for (long long b = rlen[s]; b < 4 * dwords; b++) if (rbsp[at[s] + b]) ok = 0;                   /* nothing behind the trailing bits */
            for (long long b = at[s] + 4 * dwords; b < next; b++) if (rbsp[b] != 0xA5) ok = 0;             /* the room between two slices stays untouched */
            if (!rbsp[at[s] + rlen[s] - 1] || (q[n] + 8) / 8 != rlen[s]) ok = 0;                           /* the stop bit is in the last byte */
            if (s) for (long long b = 0; b + 2 < rlen[s]; b++) emul_later |= rbsp[at[s] + b] == 0 && rbsp[at[s] + b + 1] == 0 && rbsp[at[s] + b + 2] <= 3;
            /* (c) the length pass: the writer's walk with the stores suppressed, against the count by hand; it stores nothing (dst NULL) */
            long long len = -1;
            if (idr_unit_walk(O, win, rbsp + at[s], rlen[s], nal_byte, 1, NULL, 0, 1, &len) || len != unit_bytes(rbsp + at[s], rlen[s])) ok = 0;
            ulen[s] = len;
            if (len > idr_bound(n, 1)) ok = 0;
        }
        long long total = 0, none = -1;
        if (idr_place(ulen, uoff, S, idr_bound_slices(c.mb_w, c.mb_h, c.slice_rows, 1), &total) || total < 5 * S) ok = 0;
        /* one byte less in total: refused, and the sequence of the kernels writes no unit -- the block stays as it was */
        if (idr_place(ulen, uoff, S, total - 1, &none) != PCAMV_ENOMEM || none != 0) ok = 0;
        if (idr_place(ulen, uoff, S, total, &none) || none != total) ok = 0;
        /* the units into one block of exactly the total, in two orders; after every unit nothing but its own bytes may have changed */
        int mask = 0;
        for (int s = 1; s < S; s++) mask |= 1 << (uoff[s] & 3);
        uint8_t *blocks[2] = {(uint8_t *)malloc((size_t)total), (uint8_t *)malloc((size_t)total)};
        for (int order = 0; order < 2 && ok; order++) {
            uint8_t *blk = blocks[order];
            std::vector<uint8_t> expect((size_t)total, 0x5A);
            memset(blk, 0x5A, (size_t)total);
            std::vector<int> seq;
            if (order == 0) for (int s = S - 1; s >= 0; s--) seq.push_back(s);
            else { for (int s = 1; s < S; s += 2) seq.push_back(s); for (int s = 0; s < S; s += 2) seq.push_back(s); }
            for (int s : seq) {
                long long len = -1;
                if (idr_unit(O, win, rbsp + at[s], rlen[s], nal_byte, 1, blk + uoff[s], ulen[s], &len) || len != ulen[s]) ok = 0;
                memcpy(expect.data() + uoff[s], blk + uoff[s], (size_t)ulen[s]);
                if (memcmp(blk, expect.data(), (size_t)total)) ok = 0;                  /* a store outside the unit's own bytes */
                { uint8_t *less = (uint8_t *)malloc((size_t)ulen[s] - 1); long long l2 = -1; if (idr_unit(O, win, rbsp + at[s], rlen[s], nal_byte, 1, less, ulen[s] - 1, &l2) != PCAMV_ENOMEM || l2 != 0) ok = 0; free(less); }
            }
            for (int s = 0; s < S; s++) if (blk[uoff[s]] || blk[uoff[s] + 1] || blk[uoff[s] + 2] || blk[uoff[s] + 3] != 1 || blk[uoff[s] + 4] != nal_byte) ok = 0;
        }
        if (ok && memcmp(blocks[0], blocks[1], (size_t)total)) ok = 0;
        /* (a) the host decoder of pictures of several slices, from an exact-size copy */
        int drc = 0;
        if (ok) {
            std::vector<uint8_t> exact(blocks[0], blocks[0] + total), dy(ysz), du(ysz / 4), dv(ysz / 4);
            std::vector<uint8_t> wy(pic.rec[0], pic.rec[0] + ysz), wu(pic.rec[1], pic.rec[1] + ysz / 4), wv(pic.rec[2], pic.rec[2] + ysz / 4);
            int32_t dq = -1, did = -1, dn = -1;
            drc = pcamv_gpu_decode_idr_picture(exact.data(), exact.size(), c.mb_w, c.mb_h, &probe, c.chroma_offset, dy.data(), du.data(), dv.data(), &dq, &did, &dn);
            if (c.deblock && pcamv_gpu_deblock_intra_picture(wy.data(), wu.data(), wv.data(), c.mb_w, c.mb_h, c.qp, c.chroma_offset)) ok = 0;
            if (drc || dq != c.qp || did != c.idr_pic_id || dn != S || dy != wy || du != wu || dv != wv) ok = 0;
        }
        /* (b) every slice against the one-slice path on its rows as a picture of their own */
        for (int s = 0; s < S && ok; s++) {
            const int r0 = idr_slice_row0(c.mb_h, c.slice_rows, s), n = idr_slice_n_mb(c.mb_w, c.mb_h, c.slice_rows, s), rows = n / c.mb_w;
            const uint8_t *const part[3] = {src[0] + (size_t)16 * r0 * lw, src[1] + (size_t)8 * r0 * cw, src[2] + (size_t)8 * r0 * cw};
            Coded one(c.mb_w, rows);
            one.run(part, c.mb_w, rows, c, 0, W, tab);
            long long *p1 = (long long *)malloc(sizeof(long long) * (size_t)(n + 1)), a = shdr[s].bits;
            for (int i = 0; i < n; i++) { p1[i] = a; if (one.bits[i] < 0) ok = 0; else a += one.bits[i]; }
            p1[n] = a;
            const long long l1 = idr_rbsp_bytes(a), dwords = (l1 + 3) / 4;
            uint8_t *r1 = (uint8_t *)aligned_alloc(4, (size_t)dwords * 4);
            for (long long d = 0; d < dwords; d++) { const uint32_t v = idr_pack_dword(d, shdr[s].hdr, shdr[s].bits, p1, one.slots, n); memcpy(r1 + 4 * d, &v, 4); }
            if (l1 != rlen[s] || memcmp(r1, rbsp + at[s], (size_t)l1)) ok = 0;
            if (memcmp(one.rec[0], pic.rec[0] + (size_t)16 * r0 * lw, (size_t)256 * n) || memcmp(one.rec[1], pic.rec[1] + (size_t)8 * r0 * cw, (size_t)64 * n) ||
                memcmp(one.rec[2], pic.rec[2] + (size_t)8 * r0 * cw, (size_t)64 * n)) ok = 0;
            free(p1); free(r1);
        }
        printf("%d %d %lld %d %d %d\n", k, ok ? 0 : drc ? drc : -100, total, S, emul_later, mask);
        bad += !ok;
        fwrite(&total, 8, 1, fo); fwrite(blocks[0], 1, (size_t)total, fo);
        fwrite(pic.rec[0], 1, ysz, fo); fwrite(pic.rec[1], 1, ysz / 4, fo); fwrite(pic.rec[2], 1, ysz / 4, fo);
        free(blocks[0]); free(blocks[1]); free(win); free(O.obuf); free(ulen); free(uoff); free(rbsp); free(pre); free(shdr); free(W);
    }
    fclose(f); fclose(fo);
    free(tab);
    printf("cases %d bad %ld\n", count, bad);
    return bad ? 1 : 0;
}
