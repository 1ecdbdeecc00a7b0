/* Intra4x4 macroblocks in IDR pictures: the device coder's control code (csrc/pcamv_idr_i4x4.h on top of pcamv_idr.h -- what k_idr_mb4 runs)
 * on the CPU in the scalar form of SP_LANES, under AddressSanitizer + UBSan when tests/test_idr_i4x4_cpu.py builds it.  Per case the
 * picture is coded macroblock by macroblock in the order of the launches, anti-diagonals x + 2 y, with IdrPic::i4x4 and slice_rows set; the
 * prefix, the merge, the length pass, the placement and the units are check_idr_slices.cpp's, with every RBSP offset taken from the
 * bound of an Intra4x4 macroblock (idr_slice_rbsp_at_bits).  Required per case:
 *   (a) pcamv_gpu_decode_idr_picture2 with its flag set gives the coder's own reconstruction from the bytes (of a filtered picture: that
 *       reconstruction through pcamv_gpu_deblock_intra_picture), and without the flag refuses a picture that holds an Intra4x4 macroblock;
 *   (b) with i4x4 = 1, a picture in which the decision left every macroblock Intra16x16 is, slice by slice and bit for bit, what idr_mb in
 *       the order x + y makes of it (what check_idr_write.cpp and check_idr_slices.cpp run), reconstruction and counts included; and
 *       idr_mb4 with i4x4 = 0 in the order x + 2 y gives that always;
 *   (c) no macroblock is longer than IDR_MB_BITS_I4, whose terms are maximised here once the way swvx_block_bound maximises a block's
 *       (the longest coeff_token, trailing ones, escaped levels, total_zeros and runs of each block kind; the longest ue of the chroma
 *       mode and of the pattern's codeNum) and must come to exactly IDR_MB_BITS_I4;
 *   (d) the length pass equals the written length; a capacity of one byte less is PCAMV_ENOMEM and no byte is stored.
 *
 * usage: check_idr_i4x4 <cases.bin> <out.bin>          (the case file: tests/idr_i4x4_cases.py write_case_file)
 * prints "bound <bits>" and per case
 *   <index> <rc> <total bytes> <slices> <Intra4x4 macroblocks> <Intra16x16 macroblocks> <mask of the modes chosen>
 *   <mask over blocks 3 7 11 13 15 of those with DDL or VL> <block 5 with DDL or VL: 1 with a macroblock above-right | 2 without one, top there>
 *   <1 Intra4x4 left of Intra16x16 | 2 above it | 4 Intra16x16 left of Intra4x4 | 8 above it> <Intra4x4 cbp_luma: 1 zero | 2 neither | 4 fifteen>
 *   <an Intra4x4 macroblock with pattern 0> <a slice behind the first holds 00 00 0x> <the longest macroblock's bits>
 * and "cases <n> bad <n>"; out.bin receives per case int64 length + the units, then the coder's unfiltered reconstruction.  Exit status 1
 * on any failure, 2 for a file that is no case file. */
#include "slice_write_cavlc_host.h"
#include "pcamv_idr_i4x4.h"
#include "pcamv_mvsyntax.h"
#include "pcamv_host_tables.h"
#include <stdio.h>
#include <vector>

struct Case { int32_t mb_w, mb_h, qp, dz, qpc, chroma_offset, slice_rows, idr_pic_id, deblock, i4x4; std::vector<uint8_t> pl[3]; };

struct Coded {
    uint8_t *rec[3], *nz, *modes; uint32_t *slots; int *bits, *clamped; int n_mb;
    Coded(int mb_w, int mb_h) : n_mb(mb_w * mb_h)
    {
        const size_t ysz = (size_t)256 * n_mb;
        rec[0] = (uint8_t *)malloc(ysz); rec[1] = (uint8_t *)malloc(ysz / 4); rec[2] = (uint8_t *)malloc(ysz / 4);
        memset(rec[0], 0xA5, ysz); memset(rec[1], 0xA5, ysz / 4); memset(rec[2], 0xA5, ysz / 4);
        nz = (uint8_t *)malloc((size_t)IDR_NZ_BYTES * n_mb); slots = (uint32_t *)malloc((size_t)IDR_SLOT_DWORDS * 4 * n_mb);
        modes = (uint8_t *)malloc((size_t)IDR_MODE_BYTES * n_mb);
        bits = (int *)malloc(sizeof(int) * n_mb); clamped = (int *)malloc(sizeof(int) * n_mb);
    }
    ~Coded() { for (auto *p : rec) free(p); free(nz); free(slots); free(modes); free(bits); free(clamped); }
    IdrPic pic(const uint8_t *const src[3], int mb_w, int mb_h, const Case &c, int i4x4)
    {
        IdrPic P = {{src[0], src[1], src[2]}, {rec[0], rec[1], rec[2]}, mb_w, mb_h, c.qp, c.qpc, c.dz, nz, slots, bits, clamped, c.slice_rows};
        P.i4x4 = i4x4; P.lambda = pcamv_lambda_tab[c.qp]; P.modes = i4x4 ? modes : nullptr;
        return P;
    }
    /* the order of k_idr_mb4's launches */
    IdrPic run4(const uint8_t *const src[3], int mb_w, int mb_h, const Case &c, int i4x4, IdrWork *W, IdrWork4 *W4, const uint8_t *tab)
    {
        const IdrPic P = pic(src, mb_w, mb_h, c, i4x4);
        for (int d = 0; d < mb_w + 2 * (mb_h - 1); d++)
            for (int my = 0; my < mb_h; my++) { const int mx = d - 2 * my; if (mx >= 0 && mx < mb_w) idr_mb4(*W, *W4, P, (const uint16_t *)tab, mx, my); }
        return P;
    }
    /* the order of k_idr_mb's */
    IdrPic run16(const uint8_t *const src[3], int mb_w, int mb_h, const Case &c, IdrWork *W, const uint8_t *tab)
    {
        const IdrPic P = pic(src, mb_w, mb_h, c, 0);
        for (int d = 0; d < mb_w + mb_h - 1; d++)
            for (int my = 0; my < mb_h; my++) { const int mx = d - my; if (mx >= 0 && mx < mb_w) idr_mb(*W, P, (const uint16_t *)tab, mx, my); }
        return P;
    }
    bool same(const Coded &o) const
    {
        if (memcmp(rec[0], o.rec[0], (size_t)256 * n_mb) || memcmp(rec[1], o.rec[1], (size_t)64 * n_mb) || memcmp(rec[2], o.rec[2], (size_t)64 * n_mb)) return false;
        if (memcmp(nz, o.nz, (size_t)IDR_NZ_BYTES * n_mb) || memcmp(bits, o.bits, sizeof(int) * n_mb)) return false;
        for (int i = 0; i < n_mb; i++) for (int k = 0; k < bits[i]; k++) if (idr_take(slots + (size_t)i * IDR_SLOT_DWORDS, k, 1) != idr_take(o.slots + (size_t)i * IDR_SLOT_DWORDS, k, 1)) return false;
        return true;
    }
};

static long long unit_bytes(const uint8_t *rbsp, long long len)
{
    long long want = 5; int zeros = 0;
    for (long long q = 0; q < len; q++) { if (zeros == 2 && rbsp[q] <= 3) { want++; zeros = 0; } zeros = rbsp[q] == 0 ? zeros + 1 : 0; want++; }
    return want;
}

/* ---- (c): the terms of IDR_MB_BITS_I4, maximised over the code tables */
static int rb_max(const uint16_t *vlc, int codes, int zeros, int (*memo)[17])
{
    if (!codes || !zeros) return 0;
    if (memo[codes][zeros] >= 0) return memo[codes][zeros];
    int best = 0;
    for (int run = 0; run <= zeros; run++) {
        const int len = vlc[SV_T_RB + 16 * (zeros - 1 < 6 ? zeros - 1 : 6) + run] & 31;
        if (!len) continue;
        const int b = len + rb_max(vlc, codes - 1, zeros - run, memo);
        if (b > best) best = b;
    }
    return memo[codes][zeros] = best;
}
static int block_bound(const uint8_t *tab, int count, int dc)
{
    uint16_t vlc[SV_T_N];
    memcpy(vlc, tab, sizeof(vlc));
    int memo[17][17], best = 0;
    for (int i = 0; i < 17; i++) for (int j = 0; j < 17; j++) memo[i][j] = -1;
    for (int total = 1; total <= count; total++)
        for (int t1 = 0; t1 <= 3 && t1 <= total; t1++)
            for (int tab_i = dc ? 4 : 0; tab_i < (dc ? 5 : 4); tab_i++) {
                const int ct = vlc[SV_T_COEFF + 64 * tab_i + 4 * (total - 1) + t1] & 31;
                if (!ct) continue;
                for (int zeros = 0; zeros <= count - total; zeros++) {
                    int b = ct + t1 + 28 * (total - t1);
                    if (total < count) {
                        const int tz = vlc[dc ? SV_T_TZDC + 4 * (total - 1) + zeros : SV_T_TZ + 16 * (total - 1) + zeros] & 31;
                        if (!tz) continue;
                        b += tz;
                    }
                    b += rb_max(vlc, total - 1, zeros, memo);
                    if (b > best) best = b;
                }
            }
    return best;
}
static int ue_bits(unsigned k) { return 2 * (32 - __builtin_clz(k + 1u)) - 1; }
static int mb_bound(const uint8_t *tab)
{
    int cm = 0, pat = 0, seen[48] = {0};
    for (unsigned k = 0; k <= 3; k++) if (ue_bits(k) > cm) cm = ue_bits(k);
    for (int p = 0; p < 48; p++) { const int code = idr_cbp_intra_code(p); if (code < 0 || code > 47 || seen[code]++) return -1; if (ue_bits((unsigned)code) > pat) pat = ue_bits((unsigned)code); }
    return ue_bits(0) + 16 * 4 + cm + pat + 1 + 16 * block_bound(tab, 16, 0) + 8 * block_bound(tab, 15, 0) + 2 * block_bound(tab, 4, 1);
}

/* what an Intra4x4 macroblock's bit string says in front of its residual: the pattern (-1: the string is no Intra4x4 macroblock's) */
static int i4_pattern(const uint32_t *slot, int bits)
{
    int at = 0;
    auto get = [&](int n) { const uint32_t v = at + n <= bits ? idr_take(slot, at, n) : 0; at += n; return v; };
    auto ue = [&]() { int z = 0; while (at < bits && !get(1)) z++; return (1u << z) - 1 + (z ? get(z) : 0); };
    if (!get(1)) return -1;
    for (int b = 0; b < 16; b++) if (!get(1)) get(3);
    ue();
    const unsigned code = ue();
    for (int p = 0; p < 48; p++) if ((unsigned)idr_cbp_intra_code(p) == code) return p;
    return -1;
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
    const int nal_byte = 0x65, MBB = IDR_MB_BITS_I4;
    long bad = 0;
    const int bound = mb_bound(tab);
    printf("bound %d\n", bound);
    if (bound != IDR_MB_BITS_I4) bad++;
    for (int k = 0; k < count; k++) {
        Case c;
        if (fread(&c.mb_w, 4, 10, f) != 10) return 2;
        if (c.mb_w < 1 || c.mb_h < 1 || c.mb_w * c.mb_h > 4096 || c.slice_rows < 0 || c.i4x4 < 1 || c.i4x4 > 2 || c.qp < 0 || c.qp > 51) return 2;
        const int n_mb = c.mb_w * c.mb_h, S = idr_n_slices(c.mb_h, c.slice_rows), rps = idr_rows_per_slice(c.mb_h, c.slice_rows);
        const size_t ysz = (size_t)256 * n_mb;
        for (int i = 0; i < 3; i++) { c.pl[i].resize(i ? ysz / 4 : ysz); if (fread(c.pl[i].data(), 1, c.pl[i].size(), f) != c.pl[i].size()) return 2; }
        int ok = 1;
        IdrWork *W = (IdrWork *)malloc(sizeof(IdrWork));
        IdrWork4 *W4 = (IdrWork4 *)malloc(sizeof(IdrWork4));
        const uint8_t *const src[3] = {c.pl[0].data(), c.pl[1].data(), c.pl[2].data()};
        Coded pic(c.mb_w, c.mb_h);
        const IdrPic P = pic.run4(src, c.mb_w, c.mb_h, c, c.i4x4, W, W4, tab);
        /* the census, and (c) */
        int n4 = 0, modes = 0, trb = 0, b5 = 0, adj = 0, cbpc = 0, pat0 = 0, max_bits = 0;
        std::vector<int> is4(n_mb);
        for (int i = 0; i < n_mb; i++) {
            if (pic.bits[i] < 1 || pic.bits[i] > MBB) { ok = 0; continue; }
            if (pic.bits[i] > max_bits) max_bits = pic.bits[i];
            is4[i] = (int)idr_take(pic.slots + (size_t)i * IDR_SLOT_DWORDS, 0, 1);            /* mb_type ue(0) is the one string that begins with a 1 */
            const uint8_t *m = pic.modes + (size_t)i * IDR_MODE_BYTES;
            if (!is4[i]) { for (int b = 0; b < 16; b++) if (m[b] != 2) ok = 0; continue; }
            n4++;
            const int mx = i % c.mb_w, my = i / c.mb_w, top = my % rps > 0;
            for (int b = 0; b < 16; b++) { if (m[b] > 8) { ok = 0; continue; } modes |= 1 << m[b]; }
            const int tb[5] = {3, 7, 11, 13, 15};
            for (int q = 0; q < 5; q++) if (m[tb[q]] == 3 || m[tb[q]] == 7) trb |= 1 << q;
            if ((m[5] == 3 || m[5] == 7) && top) b5 |= mx + 1 < c.mb_w ? 1 : 2;
            const int pat = i4_pattern(pic.slots + (size_t)i * IDR_SLOT_DWORDS, pic.bits[i]);
            if (pat < 0) { ok = 0; continue; }
            int cl = 0;
            for (int b = 0; b < 16; b++) if (pic.nz[(size_t)i * IDR_NZ_BYTES + b]) cl |= 1 << (b >> 2);
            if (cl != (pat & 15)) ok = 0;                                                       /* the counts the neighbours read are the pattern's */
            cbpc |= (pat & 15) == 0 ? 1 : (pat & 15) == 15 ? 4 : 2;
            if (pat == 0) pat0 = 1;
        }
        for (int i = 0; i < n_mb; i++) {
            const int mx = i % c.mb_w, my = i / c.mb_w;
            if (mx + 1 < c.mb_w) adj |= is4[i] && !is4[i + 1] ? 1 : !is4[i] && is4[i + 1] ? 4 : 0;
            if (my + 1 < c.mb_h && (my + 1) % rps) adj |= is4[i] && !is4[i + c.mb_w] ? 2 : !is4[i] && is4[i + c.mb_w] ? 8 : 0;
        }
        if (c.i4x4 == 2 && n4 != n_mb) ok = 0;
        /* (b) */
        {
            Coded ref(c.mb_w, c.mb_h), zero(c.mb_w, c.mb_h);
            ref.run16(src, c.mb_w, c.mb_h, c, W, tab);
            zero.run4(src, c.mb_w, c.mb_h, c, 0, W, W4, tab);
            if (!zero.same(ref)) ok = 0;
            if (c.i4x4 == 1 && n4 == 0 && !pic.same(ref)) ok = 0;
        }
        /* the headers, the prefix, every slice's RBSP at its place */
        IdrSliceHdr *shdr = (IdrSliceHdr *)calloc((size_t)S, sizeof(IdrSliceHdr));
        for (int s = 0; s < S; s++)
            if (pcamv_idr_header_write3(probe, 3, c.idr_pic_id, c.qp, c.deblock, idr_slice_first_mb(c.mb_w, c.mb_h, c.slice_rows, s), shdr[s].hdr, &shdr[s].bits) ||
                shdr[s].bits > IDR_HDR_MAX_BITS) ok = 0;
        long long *pre = (long long *)malloc(sizeof(long long) * (size_t)(n_mb + S));
        if (idr_prefix_slices(P, shdr, pre)) ok = 0;
        const long long area = idr_slice_rbsp_at_bits(n_mb, S, MBB);
        uint8_t *rbsp = (uint8_t *)aligned_alloc(4, (size_t)area);
        memset(rbsp, 0xA5, (size_t)area);
        long long *ulen = (long long *)malloc(sizeof(long long) * (size_t)S), *uoff = (long long *)malloc(sizeof(long long) * (size_t)S);
        IdrOut O; uint32_t *win = (uint32_t *)malloc(256); O.obuf = (uint32_t *)malloc(SW_OBUF);
        int emul_later = 0;
        std::vector<long long> at(S), rlen(S);
        for (int s = 0; s < S && ok; s++) {
            const int fm = idr_slice_first_mb(c.mb_w, c.mb_h, c.slice_rows, s), n = idr_slice_n_mb(c.mb_w, c.mb_h, c.slice_rows, s);
            const long long *q = pre + idr_slice_pre_at(fm, s);
            at[s] = idr_slice_rbsp_at_bits(fm, s, MBB); rlen[s] = idr_rbsp_bytes(q[n]);
            const long long dwords = (rlen[s] + 3) / 4, next = idr_slice_rbsp_at_bits(fm + n, s + 1, MBB);
            if (at[s] + 4 * dwords > next || next > area) { ok = 0; continue; }
            for (long long d = 0; d < dwords; d++) { const uint32_t v = idr_pack_dword(d, shdr[s].hdr, shdr[s].bits, q, pic.slots + (size_t)fm * IDR_SLOT_DWORDS, n); memcpy(rbsp + at[s] + 4 * d, &v, 4); }
            for (long long b = at[s] + 4 * dwords; b < next; b++) if (rbsp[b] != 0xA5) ok = 0;
            if (s) for (long long b = 0; b + 2 < rlen[s]; b++) emul_later |= rbsp[at[s] + b] == 0 && rbsp[at[s] + b + 1] == 0 && rbsp[at[s] + b + 2] <= 3;
            long long len = -1;
            if (idr_unit_walk(O, win, rbsp + at[s], rlen[s], nal_byte, 1, NULL, 0, 1, &len) || len != unit_bytes(rbsp + at[s], rlen[s])) ok = 0;
            ulen[s] = len;
            if (len > idr_bound_bits(n, 1, MBB)) ok = 0;
        }
        long long total = 0, none = -1;
        uint8_t *block = NULL;
        int drc = 0;
        if (ok) {
            if (idr_place(ulen, uoff, S, idr_bound_slices_bits(c.mb_w, c.mb_h, c.slice_rows, 1, MBB), &total) || total < 5 * S) ok = 0;
            /* (d) one byte less in total: refused, and the sequence of the kernels then writes no unit */
            if (idr_place(ulen, uoff, S, total - 1, &none) != PCAMV_ENOMEM || none != 0) ok = 0;
        }
        if (ok) {
            block = (uint8_t *)malloc((size_t)total);
            memset(block, 0x5A, (size_t)total);
            for (int s = S - 1; s >= 0; s--) {
                long long len = -1;
                if (idr_unit(O, win, rbsp + at[s], rlen[s], nal_byte, 1, block + uoff[s], ulen[s], &len) || len != ulen[s]) ok = 0;
                uint8_t *less = (uint8_t *)malloc((size_t)ulen[s] - 1); long long l2 = -1;
                if (idr_unit(O, win, rbsp + at[s], rlen[s], nal_byte, 1, less, ulen[s] - 1, &l2) != PCAMV_ENOMEM || l2 != 0) ok = 0;
                free(less);
            }
        }
        /* (a) */
        if (ok) {
            std::vector<uint8_t> exact(block, block + total), dy(ysz), du(ysz / 4), dv(ysz / 4);
            std::vector<uint8_t> wy(pic.rec[0], pic.rec[0] + ysz), wu(pic.rec[1], pic.rec[1] + ysz / 4), wv(pic.rec[2], pic.rec[2] + ysz / 4);
            int32_t dq = -1, did = -1, dn = -1;
            drc = pcamv_gpu_decode_idr_picture2(exact.data(), exact.size(), c.mb_w, c.mb_h, &probe, c.chroma_offset, 1, dy.data(), du.data(), dv.data(), &dq, &did, &dn);
            if (c.deblock && pcamv_gpu_deblock_intra_picture(wy.data(), wu.data(), wv.data(), c.mb_w, c.mb_h, c.qp, c.chroma_offset)) ok = 0;
            if (drc || dq != c.qp || did != c.idr_pic_id || dn != S || dy != wy || du != wu || dv != wv) ok = 0;
            const int rc0 = pcamv_gpu_decode_idr_picture(exact.data(), exact.size(), c.mb_w, c.mb_h, &probe, c.chroma_offset, dy.data(), du.data(), dv.data(), &dq, &did, &dn);
            if (n4 ? rc0 != PCAMV_EUNSUP : rc0 != 0) ok = 0;
        }
        printf("%d %d %lld %d %d %d %d %d %d %d %d %d %d %d\n", k, ok ? 0 : drc ? drc : -100, total, S, n4, n_mb - n4, modes, trb, b5, adj, cbpc, pat0, emul_later, max_bits);
        bad += !ok;
        fwrite(&total, 8, 1, fo); if (block) fwrite(block, 1, (size_t)total, fo);
        fwrite(pic.rec[0], 1, ysz, fo); fwrite(pic.rec[1], 1, ysz / 4, fo); fwrite(pic.rec[2], 1, ysz / 4, fo);
        free(block); free(win); free(O.obuf); free(ulen); free(uoff); free(rbsp); free(pre); free(shdr); free(W); free(W4);
    }
    fclose(f); fclose(fo);
    free(tab);
    printf("cases %d bad %ld\n", count, bad);
    return bad ? 1 : 0;
}
