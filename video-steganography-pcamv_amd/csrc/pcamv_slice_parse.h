/*
 * pcamv_slice_parse.h -- the CABAC P-slice parser as control code that compiles for the device and for the host.
 *
 * On the device it is the body of k_parse_pslice (pcamv_slice.hip.h): one wavefront per slice, control wave-uniform, the lanes
 * doing what is parallel -- the refill of the byte window, the context initialisation, the gather of a macroblock's
 * neighbourhood, the MV fill of a partition and the store of the record.  On the host it is what tests/emu/slice_parse_driver.cpp
 * and tests/fuzz/fuzz_slice_parse.cpp compile with scalar primitives (SP_LANES is then a loop over the 64 lanes), to be compared
 * record by record and return code by return code with the library's host parser, pcamv_mvsyntax.h, which stays the independent
 * check: nothing here is shared with it but the standard's tables.  No HIP type, no table of its own (SpTables points at
 * pcamv_entropy_tables.h's, or at their copy on the device).
 *
 * What it reads is what mvsyntax::Parser::run reads (H.264 7.3.5, 9.3): mb_skip_flag, mb_type, sub_mb_type, mvd with its
 * neighbour-dependent contexts, coded_block_pattern, mb_qp_delta, residual_block_cabac of categories 2 / 3 / 4 (decoded only to
 * keep the engine in step), end_of_slice_flag; MV prediction of 8.4.1.  Frame macroblocks, one reference, 4x4 transform,
 * cabac_init_idc 0; an intra macroblock is PCAMV_EUNSUP, a slice that ends in the wrong place, runs out of bytes or has bad
 * alignment bits PCAMV_EINVAL.
 *
 * The input is arbitrary bytes from outside.  Every loop is bounded (mb_qp_delta 104, UEGk 24 + 25, level prefix 14, 16
 * coefficients), every byte read is checked against the slice's end (sp_next_byte / sp_refill), every context index is a constant
 * plus a bounded increment below SP_NCTX, every table index is masked to its table, every cache position comes from constants.
 *
 * Working memory of one slice (SpState): LDS of the wave on the device, exact-size heap blocks in the host drivers.
 *   win   64 dwords of slice bytes, refilled by one 64-lane load
 *   ctx   the SP_NCTX context states a P slice of this path touches
 *   cmv / cmvd / cref / cnz   one macroblock's neighbourhood in x264's cache layout (8 columns; row 0 = the line above, column 3 =
 *         the column to the left), 48 positions each
 *   row   what the macroblocks of the next row read of this one, SP_ROW_BYTES per macroblock column -- the bottom row's four MVs,
 *         its coded_block_flags (luma 4, Cb 2, Cr 2), its mvds, cbp, type: the SP_ROW_* layout -- overwritten column by column as the
 *         slice advances; the macroblock to the left is still in the cache when its neighbour is gathered.  No whole-picture field.
 *
 * Stated here once: the row layout and SP_LDS_COLS for all four slice coders; for the CABAC pair (this parser, pcamv_slice_write.h)
 * sp_gather, sp_hand_on, sp_fill_pskip and sp_init_contexts; for the writer sp_partition.  The CAVLC coders keep their own gather and
 * hand-on (DESIGN.md 3g gives the measurement).  Each coder keeps its own syntax and entropy code.
 */
#ifndef PCAMV_SLICE_PARSE_H
#define PCAMV_SLICE_PARSE_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/pcamv_gpu.h"

#if defined(__HIPCC__)
#define SP_HD __host__ __device__ static inline
#else
#define SP_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
/* the body runs once per lane; a value a lane keeps from one SP_LANES block to the next is its own register */
#define SP_LANES(l) for (int l = (int)(threadIdx.x & 63u), l##_once = 1; l##_once; l##_once = 0)
#define SP_SLOTS 1
#define SP_SLOT(l) 0
/* lanes exchange data through the working memory: pins the order for the compiler, emits no instruction (PCAMV_WAVE_SYNC) */
#define SP_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                       __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#define SP_UNI(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))     /* what every lane computed alike, as a scalar */
#else
#define SP_LANES(l) for (int l = 0; l < 64; l++)
#define SP_SLOTS 64
#define SP_SLOT(l) (l)
#define SP_SYNC() do { } while (0)
#define SP_UNI(v) ((uint32_t)(v))
#endif

#define SP_NCTX 276             /* contexts 0..275 (PCAMV_CAB_USED): coeff_abs_level_minus1 of category 4 ends at 275 */
#define SP_CTX_BYTES 320
/* One column of the row buffer.  A CAVLC coder keeps the first SV_ROW_BYTES of it (cnz then holds total_coeffs), a CABAC coder all. */
enum { SP_ROW_MV = 0,           /* the bottom row's four MVs */
       SP_ROW_NZ = 16,          /* its flags or counts: luma 4, Cb 2, Cr 2 */
       SP_ROW_MVD = 24,         /* its four mvds */
       SP_ROW_CBP = 40,         /* cbp_luma | cbp_chroma << 4 | chroma DC flags << 8, two bytes */
       SP_ROW_TYPE = 42 };
#define SP_ROW_BYTES 48
#define SV_ROW_BYTES 24
static_assert(SV_ROW_BYTES == SP_ROW_MVD, "the CAVLC column is the prefix of the CABAC column that ends where the mvds begin");
static_assert(SP_ROW_TYPE < SP_ROW_BYTES && SP_ROW_MV % 4 == 0 && SP_ROW_MVD % 4 == 0, "MVs and mvds are stored as dwords");
#define SP_LDS_COLS 128         /* pictures up to this many macroblocks wide keep the row buffer in LDS (the kernels of all four coders) */
#define SP_MAX_LEN (1 << 30)    /* bytes of one slice (positions are ints) */
/* the standard's tables as one block, the form the device gets them in: context initialisers (m, n) of the first SP_NCTX contexts,
 * the state transitions, rangeTabLPS in the 128-state form */
enum { SP_TAB_INIT = 0, SP_TAB_TRANS = 2 * SP_NCTX, SP_TAB_RLPS = SP_TAB_TRANS + 256, SP_TAB_BYTES = SP_TAB_RLPS + 512 };
struct SpTables { const int8_t *init_p; const uint8_t *trans, *rlps; };

struct SpState {
    const uint8_t *src; int len;        /* slice data from the first mb_skip_flag on */
    uint32_t *win; int win_base;        /* win[k] = bytes win_base + 4 k .. + 3 of src (zeros outside the slice) */
    uint8_t *ctx;
    const uint8_t *trans, *rlps;
    uint32_t *cmv, *cmvd;               /* mvx | mvy << 16 */
    int8_t *cref;                       /* 0 = predicted from the one reference, -2 = not available */
    uint8_t *cnz;                       /* coded_block_flags: luma in the motion layout, chroma at sp_nzc_pos */
    uint8_t *row;                       /* [mb_w][SP_ROW_BYTES] (CAVLC: SV_ROW_BYTES), 4-byte aligned */
    uint32_t *tl;                       /* [1] the MV above-left of the next macroblock (its row entry is overwritten before it is read) */
    uint32_t range, offset, cache;      /* cache: the low cbits bits are slice bits not yet consumed */
    int cbits, pos, overrun, partition, last_dqp, cbp_left, type_left;
};

SP_HD uint32_t sp_ld32(const void *p) { uint32_t v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4); return v; }
SP_HD void sp_st32(void *p, uint32_t v) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 4); }
SP_HD int sp_mvx(uint32_t p) { return (int16_t)(uint16_t)(p & 0xffffu); }
SP_HD int sp_mvy(uint32_t p) { return (int16_t)(uint16_t)(p >> 16); }
SP_HD uint32_t sp_pack(int x, int y) { return (uint32_t)(uint16_t)x | (uint32_t)(uint16_t)y << 16; }     /* (int16_t) of the host parser */
SP_HD int sp_abs(int v) { return v < 0 ? -v : v; }

/* ---------------------------------------------------------------- slice bytes */
/* the window moves to the dword that holds byte pos: one load per lane, a whole dword where all four bytes are inside the slice */
SP_HD void sp_refill(SpState &S)
{
    const int base = S.pos - (int)(((uintptr_t)S.src + (uintptr_t)S.pos) & 3u);
    SP_SYNC();
    SP_LANES(l) {
        const int i = base + 4 * l;
        uint32_t w = 0;
        if (i >= 0 && i + 3 < S.len) w = sp_ld32(S.src + i);
        else for (int k = 0; k < 4; k++) if (i + k >= 0 && i + k < S.len) w |= (uint32_t)S.src[i + k] << (8 * k);
        S.win[l] = w;
    }
    SP_SYNC();
    S.win_base = base;
}
SP_HD uint32_t sp_next_byte(SpState &S)
{
    if (S.pos >= S.len) { S.overrun = 1; return 0; }            /* past the end: zeros, and the slice fails */
    if ((uint32_t)(S.pos - S.win_base) >= 256u) sp_refill(S);
    const uint32_t at = (uint32_t)(S.pos - S.win_base) & 255u;
    S.pos++;
    return (S.win[at >> 2] >> (8 * (at & 3u))) & 255u;
}
SP_HD uint32_t sp_bits(SpState &S, int n)      /* the next n <= 16 bits; a byte is fetched only when a bit of it is needed */
{
    for (int k = 0; k < 2 && S.cbits < n; k++) { S.cache = S.cache << 8 | sp_next_byte(S); S.cbits += 8; }
    S.cbits -= n;
    return SP_UNI((S.cache >> S.cbits) & ((1u << n) - 1u));
}

/* ---------------------------------------------------------------- arithmetic decoding engine (9.3.3.2) */
SP_HD void sp_renorm(SpState &S)
{
    if (S.range >= 256u) return;
    const int n = __builtin_clz(S.range | 1u) - 23;         /* range >= 6: n <= 6 (8 at most, whatever range is) */
    S.range <<= n;
    S.offset = S.offset << n | sp_bits(S, n);
}
SP_HD int sp_decision(SpState &S, int ctx)
{
    const uint32_t s = S.ctx[ctx] & 127u;
    const uint32_t rlps = S.rlps[(4u * s + ((S.range >> 6) & 3u)) & 511u];
    uint32_t b = s >> 6;
    S.range -= rlps;
    if (S.offset >= S.range) { b ^= 1u; S.offset -= S.range; S.range = rlps; }
    S.ctx[ctx] = S.trans[(2u * s + b) & 255u];
    sp_renorm(S);
    return (int)b;
}
SP_HD int sp_bypass(SpState &S)
{
    S.offset = S.offset << 1 | sp_bits(S, 1);
    if (S.offset >= S.range) { S.offset -= S.range; return 1; }
    return 0;
}
SP_HD int sp_terminal(SpState &S)
{
    S.range -= 2;
    if (S.offset >= S.range) return 1;
    sp_renorm(S);
    return 0;
}
SP_HD int sp_ue_bypass(SpState &S, int k)      /* Exp-Golomb suffix of UEGk (9.3.2.3): at most 24 + 25 bins */
{
    int v = 0;
    for (int i = 0; i < 26 && sp_bypass(S); i++) { v += 1 << k; if (++k > 24) { S.overrun = 1; break; } }
    for (int i = 0; i < 26 && k > 0; i++) { k--; v += sp_bypass(S) << k; }
    return v;
}

/* ---------------------------------------------------------------- MV prediction (8.4.1) on the cache */
enum { SP_S8_0 = 4 + 1 * 8 };
SP_HD int sp_blk_x(int idx) { return (idx & 1) | ((idx >> 1) & 2); }
SP_HD int sp_blk_y(int idx) { return ((idx >> 1) & 1) | ((idx >> 2) & 2); }
SP_HD int sp_s8(int idx) { return SP_S8_0 + sp_blk_x(idx & 15) + 8 * sp_blk_y(idx & 15); }
SP_HD int sp_med3(int a, int b, int c) { const int mn = a < b ? a : b, mx = a < b ? b : a; return mn > c ? mn : (mx < c ? mx : c); }
/* position of the coded_block_flag of block idx (0..15 luma, 16..19 Cb, 20..23 Cr) */
SP_HD int sp_nzc_pos(int idx)
{
    if (idx < 16) return sp_s8(idx);
    return 1 + ((idx - 16) & 1) + 8 * (1 + (((idx - 16) >> 1) & 1) + 3 * (((idx - 16) >> 2) & 1));
}
SP_HD void sp_predict_from3(int refa, int refb, int refc, uint32_t a, uint32_t b, uint32_t c, int mvp[2])
{
    const int cnt = (refa == 0) + (refb == 0) + (refc == 0);
    if (cnt == 1) { const uint32_t s = refa == 0 ? a : refb == 0 ? b : c; mvp[0] = sp_mvx(s); mvp[1] = sp_mvy(s); }
    else if (cnt == 0 && refb == -2 && refc == -2 && refa != -2) { mvp[0] = sp_mvx(a); mvp[1] = sp_mvy(a); }
    else { mvp[0] = sp_med3(sp_mvx(a), sp_mvx(b), sp_mvx(c)); mvp[1] = sp_med3(sp_mvy(a), sp_mvy(b), sp_mvy(c)); }
}
/* 8.4.1.3 for the partition whose first 4x4 block is idx, `width` blocks wide */
SP_HD void sp_predict_mv(const SpState &S, int idx, int width, int mvp[2])
{
    const int i8 = sp_s8(idx);                  /* 12..39: i8 - 9 >= 3, i8 - 8 + width <= 35 */
    int refa = S.cref[i8 - 1], refb = S.cref[i8 - 8], refc = S.cref[i8 - 8 + width];
    uint32_t a = S.cmv[i8 - 1], b = S.cmv[i8 - 8], c = S.cmv[i8 - 8 + width];
    if ((idx & 3) == 3 || (width == 2 && (idx & 3) == 2) || refc == -2) { refc = S.cref[i8 - 8 - 1]; c = S.cmv[i8 - 8 - 1]; }
    if (S.partition == PCAMV_D_16x8) {
        if (idx == 0 && refb == 0) { mvp[0] = sp_mvx(b); mvp[1] = sp_mvy(b); return; }
        if (idx != 0 && refa == 0) { mvp[0] = sp_mvx(a); mvp[1] = sp_mvy(a); return; }
    } else if (S.partition == PCAMV_D_8x16) {
        if (idx == 0 && refa == 0) { mvp[0] = sp_mvx(a); mvp[1] = sp_mvy(a); return; }
        if (idx != 0 && refc == 0) { mvp[0] = sp_mvx(c); mvp[1] = sp_mvy(c); return; }
    }
    sp_predict_from3(refa, refb, refc, a, b, c, mvp);
}
SP_HD void sp_predict_pskip(const SpState &S, int mv[2])          /* 8.4.1.1 */
{
    const int refa = S.cref[SP_S8_0 - 1], refb = S.cref[SP_S8_0 - 8];
    const uint32_t a = S.cmv[SP_S8_0 - 1], b = S.cmv[SP_S8_0 - 8];
    if (refa == -2 || refb == -2 || (refa == 0 && a == 0) || (refb == 0 && b == 0)) { mv[0] = mv[1] = 0; return; }
    int refc = S.cref[SP_S8_0 - 8 + 4];
    uint32_t c = S.cmv[SP_S8_0 - 8 + 4];
    if (refc == -2) { refc = S.cref[SP_S8_0 - 8 - 1]; c = S.cmv[SP_S8_0 - 8 - 1]; }
    sp_predict_from3(refa, refb, refc, a, b, c, mv);
}

/* ---------------------------------------------------------------- the neighbourhood of the CABAC coders (this parser, pcamv_slice_write.h) */
/* The gather, one cache position per lane: the column to the left out of the cache as the last macroblock left it, the line above out
 * of column rt of the row buffer, above-left from tl; everything else not available (MV, mvd and flag 0, reference -2) */
SP_HD void sp_gather(SpState &S, const uint8_t *rt, bool left, bool top, bool topright)
{
    uint32_t g_mv[SP_SLOTS], g_mvd[SP_SLOTS], g_nz[SP_SLOTS]; int g_ref[SP_SLOTS];
    SP_SYNC();
    SP_LANES(q) if (q < 48) {
        uint32_t mv = 0, mvd = 0, nz = 0; int ref = -2;
        const int col = q & 7, r = q >> 3;
        if (left && col == 3 && r >= 1 && r <= 4) { mv = S.cmv[q + 4]; mvd = S.cmvd[q + 4]; nz = S.cnz[q + 4]; ref = 0; }
        if (left && (q == 8 || q == 16 || q == 32 || q == 40)) nz = S.cnz[q + 2];
        if (top && q >= 4 && q < 8) { mv = sp_ld32(rt + SP_ROW_MV + 4 * (q - 4)); mvd = sp_ld32(rt + SP_ROW_MVD + 4 * (q - 4)); nz = rt[SP_ROW_NZ + q - 4]; ref = 0; }
        if (top && (q == 1 || q == 2)) nz = rt[SP_ROW_NZ + 4 + q - 1];
        if (top && (q == 25 || q == 26)) nz = rt[SP_ROW_NZ + 6 + q - 25];
        if (left && top && q == 3) { mv = S.tl[0]; ref = 0; }
        if (topright && q == 8) { mv = sp_ld32(rt + SP_ROW_BYTES + SP_ROW_MV); ref = 0; }
        g_mv[SP_SLOT(q)] = mv; g_mvd[SP_SLOT(q)] = mvd; g_nz[SP_SLOT(q)] = nz; g_ref[SP_SLOT(q)] = ref;
    }
    SP_SYNC();
    SP_LANES(q) if (q < 48) { S.cmv[q] = g_mv[SP_SLOT(q)]; S.cmvd[q] = g_mvd[SP_SLOT(q)]; S.cnz[q] = (uint8_t)g_nz[SP_SLOT(q)]; S.cref[q] = (int8_t)g_ref[SP_SLOT(q)]; }
    SP_SYNC();
}
/* The hand-on to the next row: the macroblock's bottom row, cbp and type into column rt once the MV above-left of the next macroblock is
 * out of it.  rec (the parser's; NULL in the writer): the macroblock's record leaves in the same pass, one dword per lane -- type,
 * S.partition, sub, the sixteen MVs of the cache, skip_mv */
SP_HD void sp_hand_on(SpState &S, uint8_t *rt, bool top, int cbp, int type, uint32_t *rec, uint32_t sub, uint32_t skip_mv)
{
    const uint32_t next_tl = top ? sp_ld32(rt + SP_ROW_MV + 12) : 0u;
    SP_SYNC();
    SP_LANES(l) {
        if (rec && l < 59)
            rec[l] = l == 0 ? (uint32_t)type : l == 1 ? (uint32_t)S.partition : l == 3 ? sub : l >= 8 && l < 24 ? S.cmv[sp_s8(l - 8)] : l == 56 ? skip_mv : 0u;
        if (l < 4) { sp_st32(rt + SP_ROW_MV + 4 * l, S.cmv[36 + l]); sp_st32(rt + SP_ROW_MVD + 4 * l, S.cmvd[36 + l]); rt[SP_ROW_NZ + l] = S.cnz[36 + l]; }
        else if (l < 8) rt[SP_ROW_NZ + l] = S.cnz[l < 6 ? 17 + (l - 4) : 41 + (l - 6)];
        else if (l == 8) { rt[SP_ROW_CBP] = (uint8_t)(cbp & 255); rt[SP_ROW_CBP + 1] = (uint8_t)(cbp >> 8); rt[SP_ROW_TYPE] = (uint8_t)type; }
    }
    SP_SYNC();
    S.tl[0] = next_tl;
}
/* a P_SKIP macroblock's motion: the prediction of 8.4.1.1 (returned in mv) into its sixteen blocks */
SP_HD void sp_fill_pskip(SpState &S, int mv[2])
{
    sp_predict_pskip(S, mv);
    const uint32_t p = SP_UNI(sp_pack(mv[0], mv[1]));
    SP_SYNC();
    SP_LANES(l) if (l < 16) { S.cmv[sp_s8(l)] = p; S.cref[sp_s8(l)] = 0; }
    SP_SYNC();
}
/* Partition k of a macroblock in syntax order as first block | width << 8 | height << 16 (in 4x4 blocks), -1 behind the last: the
 * writer's walk is ONE loop around ONE call of its mvd coder, where fifteen call sites had that coder inlined fifteen times.  sub: the
 * four sub-partitions, one byte each, 0..3 (read for P_8x8 only).  Straight-line code: a slice is one wave's serial walk, and what
 * does not depend on k leaves the loop. */
static_assert(PCAMV_D_L0_4x4 == 0 && PCAMV_D_L0_8x4 == 1 && PCAMV_D_L0_4x8 == 2 && PCAMV_D_L0_8x8 == 3, "sp_partition computes with the sub-types' values");
SP_HD int sp_partition(int type, int partition, uint32_t sub, int k)
{
    if (type != PCAMV_P_8x8) {
        const int n = partition == PCAMV_D_16x16 ? 1 : partition == PCAMV_D_16x8 || partition == PCAMV_D_8x16 ? 2 : 0;
        if ((unsigned)k >= (unsigned)n) return -1;
        return (partition == PCAMV_D_16x8 ? 8 * k : 4 * k) | (partition == PCAMV_D_8x16 ? 2 : 4) << 8 | (partition == PCAMV_D_16x8 ? 2 : 4) << 16;
    }
    /* an 8x8 of sub-type t has 4 >> ((t + 1) >> 1) = 4, 2, 2, 1 partitions; ends: the running totals behind each 8x8, one byte each */
    uint32_t ends = 0, n = 0;
    for (int i = 0; i < 4; i++) { n += 4u >> ((((sub >> (8 * i)) & 3u) + 1u) >> 1); ends |= n << (8 * i); }
    if ((unsigned)k >= n) return -1;
    const int i = (k >= (int)(ends & 255u)) + (k >= (int)((ends >> 8) & 255u)) + (k >= (int)((ends >> 16) & 255u));
    const int t = (int)((sub >> (8 * i)) & 3u), j = k - (int)(((ends << 8) >> (8 * i)) & 255u);      /* j: its place inside 8x8 i */
    return (4 * i + (t == PCAMV_D_L0_8x4 ? 2 * j : j)) | (1 + (t & 1)) << 8 | (1 + (t >> 1)) << 16;
}
/* the first n_ctx context states at the slice start from the slice QP (pcamv_build_cabac_init), one per lane per pass */
SP_HD void sp_init_contexts(SpState &S, const SpTables &T, int qp, int n_ctx)
{
    SP_SYNC();
    for (int p = 0; p < (n_ctx + 63) / 64; p++)
        SP_LANES(l) {
            const int i = 64 * p + l;
            if (i < n_ctx) {
                const int v = ((T.init_p[2 * i] * qp) >> 4) + T.init_p[2 * i + 1];
                S.ctx[i] = (uint8_t)(v < 1 ? 1 : v > 126 ? 126 : v);
            }
        }
    SP_SYNC();
}

/* ---------------------------------------------------------------- macroblock layer */
SP_HD int sp_mvd_cpn(SpState &S, int idx, int l)
{
    const int i8 = sp_s8(idx);
    const uint32_t pa = S.cmvd[i8 - 1], pb = S.cmvd[i8 - 8];
    const int amvd = l ? sp_abs(sp_mvy(pa)) + sp_abs(sp_mvy(pb)) : sp_abs(sp_mvx(pa)) + sp_abs(sp_mvx(pb));
    const int base = l ? 47 : 40;
    if (!sp_decision(S, base + (amvd > 2) + (amvd > 32))) return 0;
    int a = 1;
    while (a < 9 && sp_decision(S, base + (a + 2 < 6 ? a + 2 : 6))) a++;
    if (a == 9) a += sp_ue_bypass(S, 3);
    return sp_bypass(S) ? -a : a;
}
/* the mvd of one partition (first block idx, width x height blocks, each 1, 2 or 4), its MV into every block of it */
SP_HD void sp_mvd(SpState &S, int idx, int width, int height)
{
    int mvp[2];
    sp_predict_mv(S, idx, width, mvp);
    const int dx = sp_mvd_cpn(S, idx, 0), dy = sp_mvd_cpn(S, idx, 1);
    const uint32_t mv = sp_pack(mvp[0] + dx, mvp[1] + dy), md = sp_pack(dx, dy);
    const int lw = width == 4 ? 2 : width == 2 ? 1 : 0, q0 = sp_s8(idx);
    SP_SYNC();
    SP_LANES(l) {
        const int q = q0 + (l & (width - 1)) + 8 * (l >> lw);
        if (l < width * height && q < 48) { S.cmv[q] = mv; S.cmvd[q] = md; S.cref[q] = 0; }
    }
    SP_SYNC();
}
/* one residual block (9.3.2.5-7), decoded to keep the engine in step: returns its coded_block_flag */
SP_HD int sp_residual(SpState &S, int cat, int inc)
{
    const int sig_off = cat == 2 ? 134 : cat == 3 ? 149 : 152, last_off = cat == 2 ? 195 : cat == 3 ? 210 : 213;
    const int lvl_off = cat == 2 ? 247 : cat == 3 ? 257 : 266, cnt = cat == 3 ? 4 : cat == 4 ? 15 : 16;
    if (!sp_decision(S, 85 + 4 * cat + (inc & 3))) return 0;
    int n = 0, i;
    for (i = 0; i < cnt - 1; i++)
        if (sp_decision(S, sig_off + i)) {
            n++;
            if (sp_decision(S, last_off + i)) break;
        }
    if (i == cnt - 1) n++;
    int neq1 = 0, ngt1 = 0;
    for (int k = n - 1; k >= 0; k--) {
        const int node = ngt1 ? (3 + ngt1 < 7 ? 3 + ngt1 : 7) : (neq1 < 3 ? neq1 : 3);
        const int c1 = node < 4 ? node + 1 : 0, c2 = node < 4 ? 5 : (node + 2 < 9 ? node + 2 : 9);
        if (sp_decision(S, lvl_off + c1)) {
            int prefix = 1;
            while (prefix < 14 && sp_decision(S, lvl_off + c2)) prefix++;
            if (prefix == 14) sp_ue_bypass(S, 0);
            ngt1++;
        } else neq1++;
        sp_bypass(S);                                                   /* sign */
    }
    return 1;
}

/* the slice data at S.src: every macroblock's record into out[mb_w * mb_h] */
SP_HD int sp_run(SpState &S, int mb_w, int mb_h, pcamv_mb_t *out)
{
    S.last_dqp = 0; S.cbp_left = 0; S.type_left = 0;
    for (int my = 0; my < mb_h; my++)
        for (int mx = 0; mx < mb_w; mx++) {
            const int xy = my * mb_w + mx;
            const bool left = mx > 0, top = my > 0;
            uint8_t *rt = S.row + (size_t)SP_ROW_BYTES * mx;
            sp_gather(S, rt, left, top, top && mx < mb_w - 1);
            const int cl = left ? S.cbp_left : -1, ct = top ? (int)(rt[SP_ROW_CBP] | rt[SP_ROW_CBP + 1] << 8) : -1;
            const int tl = left ? S.type_left : -1, tt = top ? (int)rt[SP_ROW_TYPE] : -1;

            int type = PCAMV_P_L0, partition = PCAMV_D_16x16, skip_mv[2] = {0, 0};
            uint32_t sub = PCAMV_D_L0_8x8 * 0x01010101u;               /* i_sub_partition[4], one byte each */
            int cbp_luma = 0, cbp_chroma = 0, dcf = 0;
            S.partition = PCAMV_D_16x16;
            const int skip = sp_decision(S, 11 + (tl >= 0 && tl != PCAMV_P_SKIP) + (tt >= 0 && tt != PCAMV_P_SKIP));
            if (skip) {
                sp_fill_pskip(S, skip_mv);
                type = PCAMV_P_SKIP;
                S.last_dqp = 0;
            } else {
                if (sp_decision(S, 14)) return PCAMV_EUNSUP;            /* an intra macroblock in a P slice */
                if (!sp_decision(S, 15)) { if (sp_decision(S, 16)) { type = PCAMV_P_8x8; partition = PCAMV_D_8x8; } }
                else partition = sp_decision(S, 17) ? PCAMV_D_16x8 : PCAMV_D_8x16;
                S.partition = partition;
                if (type == PCAMV_P_8x8) {
                    sub = 0;
                    for (int i = 0; i < 4; i++) {
                        int t;
                        if (sp_decision(S, 21)) t = PCAMV_D_L0_8x8;
                        else if (!sp_decision(S, 22)) t = PCAMV_D_L0_8x4;
                        else t = sp_decision(S, 23) ? PCAMV_D_L0_4x8 : PCAMV_D_L0_4x4;
                        sub |= (uint32_t)t << (8 * i);
                    }
                    /* (its own walk: the loop over sp_partition cost k_parse_pslice 1.2 %, 15.785 against 15.599 ms) */
                    for (int i = 0; i < 4; i++) {
                        const int t = (int)((sub >> (8 * i)) & 255u);
                        if (t == PCAMV_D_L0_8x8) sp_mvd(S, 4 * i, 2, 2);
                        else if (t == PCAMV_D_L0_8x4) { sp_mvd(S, 4 * i, 2, 1); sp_mvd(S, 4 * i + 2, 2, 1); }
                        else if (t == PCAMV_D_L0_4x8) { sp_mvd(S, 4 * i, 1, 2); sp_mvd(S, 4 * i + 1, 1, 2); }
                        else for (int k = 0; k < 4; k++) sp_mvd(S, 4 * i + k, 1, 1);
                    }
                } else if (partition == PCAMV_D_16x16) sp_mvd(S, 0, 4, 4);
                else if (partition == PCAMV_D_16x8) { sp_mvd(S, 0, 4, 2); sp_mvd(S, 8, 4, 2); }
                else { sp_mvd(S, 0, 2, 4); sp_mvd(S, 4, 2, 4); }
                /* coded_block_pattern */
                int b;
                b = sp_decision(S, 76 - ((cl >> 1) & 1) - ((ct >> 1) & 2)); cbp_luma |= b;
                b = sp_decision(S, 76 - (cbp_luma & 1) - ((ct >> 2) & 2)); cbp_luma |= b << 1;
                b = sp_decision(S, 76 - ((cl >> 3) & 1) - ((cbp_luma << 1) & 2)); cbp_luma |= b << 2;
                b = sp_decision(S, 76 - ((cbp_luma >> 2) & 1) - (cbp_luma & 2)); cbp_luma |= b << 3;
                const int ca = cl & 0x30, cb = ct & 0x30;
                if (sp_decision(S, 77 + ((ca && cl != -1) ? 1 : 0) + ((cb && ct != -1) ? 2 : 0)))
                    cbp_chroma = 1 + sp_decision(S, 77 + 4 + (ca == 0x20) + 2 * (cb == 0x20));
                if (cbp_luma | cbp_chroma) {                            /* mb_qp_delta */
                    int n = 0;
                    if (sp_decision(S, 60 + (S.last_dqp != 0))) { n = 1; while (sp_decision(S, n == 1 ? 62 : 63)) if (++n > 104) return PCAMV_EINVAL; }
                    S.last_dqp = n ? ((n + 1) >> 1) * ((n & 1) ? 1 : -1) : 0;
                    for (int i = 0; i < 16; i++)
                        if ((cbp_luma >> (i >> 2)) & 1) {
                            const int q = sp_nzc_pos(i);
                            S.cnz[q] = (uint8_t)sp_residual(S, 2, (S.cnz[q - 1] != 0) + 2 * (S.cnz[q - 8] != 0));
                        }
                    if (cbp_chroma) {
                        for (int k = 0; k < 2; k++) {
                            const int inc = (cl != -1 ? (cl >> (8 + k)) & 1 : 0) + 2 * (ct != -1 ? (ct >> (8 + k)) & 1 : 0);
                            dcf |= sp_residual(S, 3, inc) << k;
                        }
                        if (cbp_chroma == 2)
                            for (int i = 16; i < 24; i++) {
                                const int q = sp_nzc_pos(i);
                                S.cnz[q] = (uint8_t)sp_residual(S, 4, (S.cnz[q - 1] != 0) + 2 * (S.cnz[q - 8] != 0));
                            }
                    }
                } else S.last_dqp = 0;
            }
            /* the record, and what the next macroblocks read */
            const int cbp = cbp_luma | cbp_chroma << 4 | dcf << 8;
            sp_hand_on(S, rt, top, cbp, type, (uint32_t *)(void *)(out + xy), sub, sp_pack(skip_mv[0], skip_mv[1]));
            S.cbp_left = cbp; S.type_left = type;
            const int end = sp_terminal(S);
            if (end != (xy == mb_w * mb_h - 1)) return PCAMV_EINVAL;        /* end_of_slice_flag in the wrong place */
            if (S.overrun) return PCAMV_EINVAL;
        }
    return 0;
}

/* One slice: the slice data behind bit start_bit of rbsp[len] (cabac_alignment_one_bits up to the byte boundary first), slice QP qp,
 * into out[mb_w * mb_h].  S brings the working memory (win, ctx, cmv, cmvd, cref, cnz, row, tl); T the tables, of which trans and
 * rlps are read on the serial chain (LDS copies on the device).  Returns 0, PCAMV_EINVAL or PCAMV_EUNSUP, like
 * pcamv_gpu_parse_pslice_cabac_at. */
SP_HD int pcamv_slice_parse(SpState &S, const SpTables &T, const uint8_t *rbsp, long long len, long long start_bit, int qp, int mb_w, int mb_h,
                            pcamv_mb_t *out)
{
    if (!rbsp || !out || len < 0 || len > SP_MAX_LEN || start_bit < 0 || start_bit > len * 8 || mb_w < 1 || mb_h < 1 || qp < 0 || qp > 51) return PCAMV_EINVAL;
    if (start_bit & 7) {                            /* cabac_alignment_one_bit: the rest of this byte is ones */
        const uint32_t ones = 0xffu >> (start_bit & 7);
        if ((rbsp[start_bit >> 3] & ones) != ones) return PCAMV_EINVAL;
        start_bit = (start_bit | 7) + 1;
    }
    S.src = rbsp + (start_bit >> 3); S.len = (int)(len - (start_bit >> 3));
    if (S.len < 2) return PCAMV_EINVAL;
    S.trans = T.trans; S.rlps = T.rlps;
    sp_init_contexts(S, T, qp, SP_NCTX);
    S.pos = 0; S.win_base = -1024; S.cache = 0; S.cbits = 0; S.overrun = 0;
    S.range = 510; S.offset = sp_bits(S, 9);
    return sp_run(S, mb_w, mb_h, out);
}
#endif
