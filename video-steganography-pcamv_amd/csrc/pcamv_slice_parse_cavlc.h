/*
 * pcamv_slice_parse_cavlc.h -- the CAVLC P-slice parser as control code that compiles for the device and for the host.
 *
 * The --no-cabac counterpart of pcamv_slice_parse.h, under the same rules: on the device the body of k_parse_pslice_cavlc
 * (pcamv_slice.hip.h), one wavefront per slice, control wave-uniform; on the host what tests/emu/slice_parse_cavlc_driver.cpp and
 * tests/fuzz/fuzz_slice_parse_cavlc.cpp compile with scalar primitives, to be compared record by record and return code by return
 * code with the library's host parser mvsyntax::ParserV (pcamv_mvsyntax.h), which stays the independent check: the two share
 * nothing but the standard's tables.  From pcamv_slice_parse.h it takes the byte window and its refill, the MV prediction on the
 * macroblock cache and the packing helpers.  No HIP type.
 *
 * What it reads is what ParserV::run reads (H.264 7.3.5, 9.2): mb_skip_run, mb_type (ue; above 4 = intra = PCAMV_EUNSUP),
 * sub_mb_type, mvd as se pairs with the prediction of 8.4.1, coded_block_pattern through the inverse of
 * pcamv_inter_cbp_to_golomb, mb_qp_delta, residual_block_cavlc of luma 4x4, chroma DC and chroma AC (decoded only to stay in
 * step), rbsp_slice_trailing_bits.
 *
 * The contract is the host parser's return code on every input, damaged ones included, and byte-equal records where both codes
 * are 0.  The host parser counts overruns and looks at the count once per macroblock.  Between the mb_type check and that look no
 * other code than PCAMV_EINVAL can be returned, so here a step that has overrun may stop early -- the code stays the same -- but up
 * to the mb_type check the reader behaves bit by bit like the host's: past the slice's end the bits are zeros, sv_ue gives 0 once an
 * overrun has happened, and `mb_type > 4` returns at once, overrun or not.
 *
 * What the lanes do: the window refill (one dword each), every VLC decode (one table entry per lane, sv_vlc), the gather of the
 * neighbourhood (one cache position each), the MV fill of a partition, the store of the record and of the row buffer.
 *
 * The input is arbitrary bytes from outside.  Every loop is bounded (16 coefficients, level_prefix 32, 25 zeros of an Exp-Golomb
 * prefix, the trailing bits one dword a step), every byte read is checked against the slice's end (sp_refill), every table index
 * is masked or comes from a bounded count, every cache position comes from constants.
 *
 * Working memory of one slice (SvState): LDS of the wave on the device, exact-size heap blocks in the host drivers.
 *   win   64 dwords of slice bytes, refilled by one 64-lane load
 *   vlc / cbp_of   the tables (SV_T_*)
 *   cmv / cref / cnz   one macroblock's neighbourhood in x264's cache layout, 48 positions each; cnz holds total_coeff,
 *         0x80 = not available
 *   row   what the macroblocks of the next row read of this one, SV_ROW_BYTES per macroblock column: the bottom row's four MVs
 *         (SP_ROW_MV) and its eight total_coeffs (SP_ROW_NZ: luma 4, Cb 2, Cr 2).  The type of the macroblock above is not kept:
 *         no CAVLC syntax element of a P slice depends on it (a skipped macroblock above counts through its total_coeffs, 0).
 */
#ifndef PCAMV_SLICE_PARSE_CAVLC_H
#define PCAMV_SLICE_PARSE_CAVLC_H
#include "pcamv_slice_parse.h"
#include "pcamv_entropy_tables.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define SV_BALLOT(hit, l) ((uint64_t)__builtin_amdgcn_ballot_w64(hit))     /* every lane gets the whole mask */
#else
#define SV_BALLOT(hit, l) ((uint64_t)((hit) ? 1 : 0) << (l))               /* ... or adds its bit, SP_LANES being a loop */
#endif

/* The VLC tables as one block, the form the device gets them in.  One 16-bit entry per code: len | code << 5 (len 0: no such
 * code).  coeff_token: 5 classes (nC 0-1, 2-3, 4-7, 8+, chroma DC) of 64 entries, entry 4 (total_coeff - 1) + trailing_ones, and
 * entry 3 -- a slot no token has -- the class's total_coeff = 0 code.  total_zeros: 15 rows of 16; for chroma DC 3 rows of 4;
 * run_before: 7 rows of 16.  Behind them, as bytes, codeNum -> coded_block_pattern of an inter macroblock. */
enum { SV_T_COEFF = 0, SV_T_TZ = 5 * 64, SV_T_TZDC = SV_T_TZ + 15 * 16, SV_T_RB = SV_T_TZDC + 16, SV_T_N = SV_T_RB + 7 * 16,
       SV_T_CBP = 2 * SV_T_N, SV_TAB_BYTES = SV_T_CBP + 48, SV_COEFF0_SLOT = 3 };

struct SvState : SpState {
    const uint16_t *vlc;                /* SV_T_N entries */
    const uint8_t *cbp_of;              /* 48 */
    long long nbits, bp;                /* bits of the RBSP handed over, the bit the reader stands at */
};

/* host side: tab[SV_TAB_BYTES] from the arrays of pcamv_entropy_tables.h; non-zero if a code does not fit an entry */
static inline int sv_build_tables(uint8_t *tab)
{
    uint16_t e[SV_T_N];
    int bad = 0;
    auto put = [&](int at, int len, int code) { bad |= len < 0 || len > 16 || code < 0 || code >= 2048 || (len < 16 && code >> len); e[at] = (uint16_t)(len | code << 5); };
    for (int i = 0; i < SV_T_N; i++) e[i] = 0;
    for (int t = 0; t < 5; t++) {
        for (int k = 0; k < 64; k++) put(SV_T_COEFF + 64 * t + k, pcamv_vlc_coeff_len[64 * t + k], pcamv_vlc_coeff_code[64 * t + k]);
        bad |= pcamv_vlc_coeff_len[64 * t + SV_COEFF0_SLOT] != 0;
        put(SV_T_COEFF + 64 * t + SV_COEFF0_SLOT, pcamv_vlc_coeff0_len[t], pcamv_vlc_coeff0_code[t]);
    }
    for (int k = 0; k < 15 * 16; k++) put(SV_T_TZ + k, pcamv_vlc_total_zeros_len[k], pcamv_vlc_total_zeros_code[k]);
    for (int k = 0; k < 12; k++) put(SV_T_TZDC + k, pcamv_vlc_total_zeros_dc_len[k], pcamv_vlc_total_zeros_dc_code[k]);
    for (int k = 0; k < 7 * 16; k++) put(SV_T_RB + k, pcamv_vlc_run_before_len[k], pcamv_vlc_run_before_code[k]);
    __builtin_memcpy(tab, e, sizeof(e));
    for (int i = 0; i < 48; i++) tab[SV_T_CBP + i] = 0;
    for (int i = 0; i < 48; i++) { bad |= pcamv_inter_cbp_to_golomb[i] > 47; tab[SV_T_CBP + (pcamv_inter_cbp_to_golomb[i] & 63) % 48] = (uint8_t)i; }
    return bad;
}

/* ---------------------------------------------------------------- bit reader on the byte window */
/* the next 32 bits at any bit position, zeros past the slice's end */
SP_HD uint32_t sv_peek(SvState &S)
{
    const int byte = (int)(S.bp >> 3);
    if ((uint32_t)(byte - S.win_base) > 251u) { S.pos = byte; sp_refill(S); }          /* bytes byte .. byte + 4 inside the window */
    const uint32_t at = (uint32_t)(byte - S.win_base) & 255u, d = (at >> 2) & 63u, d1 = d < 63u ? d + 1u : 63u;
    const uint64_t two = (uint64_t)__builtin_bswap32(S.win[d]) << 32 | __builtin_bswap32(S.win[d1]);
    return SP_UNI((uint32_t)((two << (8u * (at & 3u) + (uint32_t)(S.bp & 7))) >> 32));
}
SP_HD void sv_skip(SvState &S, int n)           /* BitRd::get's bookkeeping */
{
    S.bp += n;
    if (S.bp > S.nbits) S.overrun = 1;
}
SP_HD uint32_t sv_get(SvState &S, int n)        /* n <= 32 */
{
    if (n <= 0) return 0;
    const uint32_t v = sv_peek(S) >> (32 - n);
    sv_skip(S, n);
    return v;
}
/* BitRd::ue: more than 24 zeros, or the end of the bits before the 1, is an overrun and gives 0; so does every call after an overrun */
SP_HD uint32_t sv_ue(SvState &S)
{
    const uint32_t p = sv_peek(S);
    if (S.overrun) { sv_skip(S, 1); return 0; }
    const int z = p ? __builtin_clz(p) : 32;
    if (z > 24) { sv_skip(S, 25); S.overrun = 1; return 0; }
    sv_skip(S, z + 1);
    return ((1u << z) - 1u) + sv_get(S, z);
}
SP_HD int sv_se(SvState &S) { const uint32_t k = sv_ue(S); return (k & 1u) ? (int)((k + 1u) >> 1) : -(int)(k >> 1); }

/* One VLC symbol: entries first .. first + n - 1 of the table, one per lane (n <= 64); the codes are prefix-free, so at most one
 * lane matches.  Returns its index and consumes its bits, or -1 and consumes nothing. */
SP_HD int sv_vlc(SvState &S, int first, int n)
{
    const uint32_t p = sv_peek(S);
    uint64_t hits = 0;
    int lens[SP_SLOTS];
    SP_LANES(l) {
        const uint32_t at = (uint32_t)(first + l), e = l < n && at < (uint32_t)SV_T_N ? S.vlc[at] : 0u, len = e & 31u;
        lens[SP_SLOT(l)] = (int)len;
        hits |= SV_BALLOT(len != 0u && (p >> ((32u - len) & 31u)) == e >> 5, l);
    }
    if (!hits) return -1;
    const int k = __builtin_ctzll(hits);
    int len = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    len = __builtin_amdgcn_readlane(lens[0], k);
#else
    len = lens[k];
#endif
    sv_skip(S, len);
    return k;
}

/* one residual block (9.2), decoded to stay in step: returns total_coeff.  tab: 0..3 by nC, 4 = chroma DC; maxc: 16, 15 or 4.
 * An error sets S.overrun and returns 0, like ParserV::residual. */
SP_HD int sv_residual(SvState &S, int tab, int maxc)
{
    if (S.overrun) return 0;                                            /* the macroblock fails whatever follows */
    const int k = sv_vlc(S, SV_T_COEFF + 64 * (tab < 4 ? tab & 3 : 4), 64);
    if (k == SV_COEFF0_SLOT) return 0;
    const int total = (k >> 2) + 1, t1 = k & 3;
    if (k < 0 || total > maxc) { S.overrun = 1; return 0; }
    int suffix_len = total > 10 && t1 < 3;
    sv_skip(S, t1);                                                     /* signs of the trailing ones */
    for (int i = t1; i < total && i < 16; i++) {
        const uint32_t p = sv_peek(S);
        if (!p || S.overrun) { S.overrun = 1; return 0; }               /* level_prefix above 31, or the bits ran out */
        const int prefix = __builtin_clz(p);
        sv_skip(S, prefix + 1);
        const int ssize = (prefix == 14 && suffix_len == 0) ? 4 : (prefix >= 15 ? prefix - 3 : suffix_len);     /* <= 28 */
        int code = ((prefix < 15 ? prefix : 15) << suffix_len) + (int)sv_get(S, ssize);
        if (prefix >= 15 && suffix_len == 0) code += 15;
        if (prefix >= 16) code += (1 << (prefix - 3)) - 4096;
        if (i == t1 && t1 < 3) code += 2;
        const int a = (code + 2) >> 1;                                  /* |level| */
        if (suffix_len == 0) suffix_len = 1;
        if (a > (3 << (suffix_len - 1)) && suffix_len < 6) suffix_len++;
    }
    int zeros = 0;
    if (total < maxc) {
        zeros = tab == 4 ? sv_vlc(S, SV_T_TZDC + 4 * ((total - 1) & 3), 4) : sv_vlc(S, SV_T_TZ + 16 * ((total - 1) & 15), 16);
        if (zeros < 0) { S.overrun = 1; return 0; }
    }
    for (int i = 0; i < total - 1 && i < 15 && zeros > 0; i++) {
        const int r = sv_vlc(S, SV_T_RB + 16 * (zeros - 1 < 6 ? zeros - 1 : 6), 16);
        if (r < 0 || r > zeros) { S.overrun = 1; return 0; }
        zeros -= r;
    }
    return total;
}
SP_HD int sv_nc_table(const SvState &S, int q)         /* the coeff_token class of the block at cache position q (9.2.1) */
{
    int nc = S.cnz[q - 1] + S.cnz[q - 8];
    if (nc < 0x80) nc = (nc + 1) >> 1;
    nc &= 0x7f;
    return nc < 2 ? 0 : nc < 4 ? 1 : nc < 8 ? 2 : 3;
}

/* the mvd of one partition (first block idx, width x height blocks, each 1, 2 or 4), its MV into every block of it */
SP_HD void sv_mvd(SvState &S, int idx, int width, int height)
{
    int mvp[2];
    sp_predict_mv(S, idx, width, mvp);
    const int dx = sv_se(S), dy = sv_se(S);
    const uint32_t mv = sp_pack(mvp[0] + dx, mvp[1] + dy);
    const int lw = width == 4 ? 2 : width == 2 ? 1 : 0, q0 = sp_s8(idx);
    SP_SYNC();
    SP_LANES(l) {
        const int q = q0 + (l & (width - 1)) + 8 * (l >> lw);
        if (l < width * height && q < 48) { S.cmv[q] = mv; S.cref[q] = 0; }
    }
    SP_SYNC();
}

/* the slice data at bit S.bp: every macroblock's record into out[mb_w * mb_h] */
SP_HD int sv_run(SvState &S, int mb_w, int mb_h, pcamv_mb_t *out)
{
    int skip_run = -1;                  /* -1: the next thing in the stream is an mb_skip_run */
    for (int my = 0; my < mb_h; my++)
        for (int mx = 0; mx < mb_w; mx++) {
            const int xy = my * mb_w + mx;
            const bool left = mx > 0, top = my > 0, topleft = left && top, topright = top && mx < mb_w - 1;
            uint8_t *rt = S.row + (size_t)SV_ROW_BYTES * mx;
            /* the neighbourhood, one cache position per lane: the column to the left out of the cache as the last macroblock left
             * it, the line above out of the row buffer; everything else not available, the macroblock's own blocks 0 */
            uint32_t g_mv[SP_SLOTS], g_nz[SP_SLOTS]; int g_ref[SP_SLOTS];
            SP_SYNC();
            SP_LANES(q) if (q < 48) {
                uint32_t mv = 0, nz = 0x80; int ref = -2;
                const int col = q & 7, r = q >> 3;
                if (left && col == 3 && r >= 1 && r <= 4) { mv = S.cmv[q + 4]; nz = S.cnz[q + 4]; ref = 0; }
                if (left && (q == 8 || q == 16 || q == 32 || q == 40)) nz = S.cnz[q + 2];
                if (top && q >= 4 && q < 8) { mv = sp_ld32(rt + SP_ROW_MV + 4 * (q - 4)); nz = rt[SP_ROW_NZ + q - 4]; ref = 0; }
                if (top && (q == 1 || q == 2)) nz = rt[SP_ROW_NZ + 4 + q - 1];
                if (top && (q == 25 || q == 26)) nz = rt[SP_ROW_NZ + 6 + q - 25];
                if (topleft && q == 3) { mv = S.tl[0]; ref = 0; }
                if (topright && q == 8) { mv = sp_ld32(rt + SV_ROW_BYTES + SP_ROW_MV); ref = 0; }
                if (col >= 4 && r >= 1 && r <= 4) nz = 0;
                if ((col == 1 || col == 2) && (r == 1 || r == 2 || r == 4 || r == 5)) nz = 0;
                g_mv[SP_SLOT(q)] = mv; g_nz[SP_SLOT(q)] = nz; g_ref[SP_SLOT(q)] = ref;
            }
            SP_SYNC();
            SP_LANES(q) if (q < 48) { S.cmv[q] = g_mv[SP_SLOT(q)]; S.cnz[q] = (uint8_t)g_nz[SP_SLOT(q)]; S.cref[q] = (int8_t)g_ref[SP_SLOT(q)]; }
            SP_SYNC();

            int type = PCAMV_P_L0, partition = PCAMV_D_16x16, skip_mv[2] = {0, 0};
            uint32_t sub = PCAMV_D_L0_8x8 * 0x01010101u;               /* i_sub_partition[4], one byte each */
            S.partition = PCAMV_D_16x16;
            if (skip_run < 0) skip_run = (int)sv_ue(S);
            if (skip_run > 0) {
                skip_run--;             /* (when the run is used up the next macroblock is a coded one: no new run is read before it) */
                sp_predict_pskip(S, skip_mv);
                const uint32_t mv = sp_pack(skip_mv[0], skip_mv[1]);
                SP_SYNC();
                SP_LANES(l) if (l < 16) { S.cmv[sp_s8(l)] = mv; S.cref[sp_s8(l)] = 0; }
                SP_SYNC();
                type = PCAMV_P_SKIP;
            } else {
                skip_run = -1;
                const uint32_t mt = sv_ue(S);
                if (mt > 4u) return PCAMV_EUNSUP;                       /* an intra macroblock in a P slice */
                if (mt >= 3u) {
                    type = PCAMV_P_8x8; partition = PCAMV_D_8x8; S.partition = PCAMV_D_8x8;
                    sub = 0;
                    for (int i = 0; i < 4; i++) {
                        const uint32_t st = sv_ue(S);
                        if (st > 3u) return PCAMV_EINVAL;
                        sub |= (uint32_t)(st == 0 ? PCAMV_D_L0_8x8 : st == 1 ? PCAMV_D_L0_8x4 : st == 2 ? PCAMV_D_L0_4x8 : PCAMV_D_L0_4x4) << (8 * i);
                    }
                    for (int i = 0; i < 4; i++) {
                        const int t = (int)((sub >> (8 * i)) & 255u);
                        if (t == PCAMV_D_L0_8x8) sv_mvd(S, 4 * i, 2, 2);
                        else if (t == PCAMV_D_L0_8x4) { sv_mvd(S, 4 * i, 2, 1); sv_mvd(S, 4 * i + 2, 2, 1); }
                        else if (t == PCAMV_D_L0_4x8) { sv_mvd(S, 4 * i, 1, 2); sv_mvd(S, 4 * i + 1, 1, 2); }
                        else for (int k = 0; k < 4; k++) sv_mvd(S, 4 * i + k, 1, 1);
                    }
                } else {
                    partition = mt == 0 ? PCAMV_D_16x16 : mt == 1 ? PCAMV_D_16x8 : PCAMV_D_8x16;
                    S.partition = partition;
                    if (mt == 0) sv_mvd(S, 0, 4, 4);
                    else if (mt == 1) { sv_mvd(S, 0, 4, 2); sv_mvd(S, 8, 4, 2); }
                    else { sv_mvd(S, 0, 2, 4); sv_mvd(S, 4, 2, 4); }
                }
                const uint32_t cn = sv_ue(S);
                if (cn > 47u) return PCAMV_EINVAL;
                const int cbp = S.cbp_of[cn % 48u], cbp_luma = cbp & 15, cbp_chroma = cbp >> 4;
                if (cbp) {
                    sv_se(S);                                           /* mb_qp_delta */
                    for (int i = 0; i < 16; i++)
                        if ((cbp_luma >> (i >> 2)) & 1) {
                            const int q = sp_nzc_pos(i);
                            S.cnz[q] = (uint8_t)sv_residual(S, sv_nc_table(S, q), 16);
                        }
                    if (cbp_chroma) {
                        sv_residual(S, 4, 4); sv_residual(S, 4, 4);
                        if (cbp_chroma & 2)
                            for (int i = 16; i < 24; i++) {
                                const int q = sp_nzc_pos(i);
                                S.cnz[q] = (uint8_t)sv_residual(S, sv_nc_table(S, q), 15);
                            }
                    }
                }
            }
            /* the record, one dword per lane; what the next macroblocks read: the bottom row into the row buffer once the MV
             * above-left of the next macroblock is out of it */
            const uint32_t next_tl = top ? sp_ld32(rt + SP_ROW_MV + 12) : 0u;
            uint32_t *o = (uint32_t *)(void *)(out + xy);
            SP_SYNC();
            SP_LANES(l) {
                if (l < 59) {
                    uint32_t v = 0;
                    if (l == 0) v = (uint32_t)type;
                    else if (l == 1) v = (uint32_t)partition;
                    else if (l == 3) v = sub;
                    else if (l >= 8 && l < 24) v = S.cmv[sp_s8(l - 8)];
                    else if (l == 56) v = sp_pack(skip_mv[0], skip_mv[1]);
                    o[l] = v;
                }
                if (l < 4) { sp_st32(rt + SP_ROW_MV + 4 * l, S.cmv[36 + l]); rt[SP_ROW_NZ + l] = S.cnz[36 + l]; }
                else if (l < 8) rt[SP_ROW_NZ + l] = S.cnz[l < 6 ? 17 + (l - 4) : 41 + (l - 6)];
            }
            SP_SYNC();
            S.tl[0] = next_tl;
            if (S.overrun) return PCAMV_EINVAL;
        }
    if (skip_run > 0) return PCAMV_EINVAL;          /* the last mb_skip_run claims more macroblocks than the picture has left */
    /* rbsp_slice_trailing_bits: a 1, then zeros to the end of the bytes handed over */
    if (S.bp >= S.nbits || !sv_get(S, 1)) return PCAMV_EINVAL;
    while (S.bp < S.nbits) {
        const long long rest = S.nbits - S.bp;
        if (sv_get(S, rest < 32 ? (int)rest : 32)) return PCAMV_EINVAL;
    }
    return 0;
}

/* One slice: the slice data from bit start_bit of rbsp[len] on (no alignment: CAVLC slice data follows the header directly), into
 * out[mb_w * mb_h].  S brings the working memory (win, cmv, cref, cnz, row, tl) and the tables (vlc, cbp_of).  Returns 0,
 * PCAMV_EINVAL or PCAMV_EUNSUP, like pcamv_gpu_parse_pslice_cavlc_at. */
SP_HD int pcamv_slice_parse_cavlc(SvState &S, const uint8_t *rbsp, long long len, long long start_bit, int mb_w, int mb_h, pcamv_mb_t *out)
{
    if (!rbsp || !out || len < 1 || len > SP_MAX_LEN || start_bit < 0 || start_bit >= len * 8 || mb_w < 1 || mb_h < 1) return PCAMV_EINVAL;
    S.src = rbsp; S.len = (int)len;
    S.nbits = len * 8; S.bp = start_bit;
    S.pos = 0; S.win_base = -1024; S.overrun = 0;
    return sv_run(S, mb_w, mb_h, out);
}
#endif
