/*
 * pcamv_stream_index.h -- the layer above a NAL unit as control code that compiles for the device and for the host: an Annex B byte
 * stream cut into its units, and the header of a P slice read.
 *
 * On the device it is the body of k_stream_scan, k_stream_prefix, k_stream_place and k_slice_header (pcamv_slice.hip.h).  On the host
 * it is what tests/fuzz/check_stream_index.cpp compiles with the scalar form of SP_LANES (pcamv_slice_parse.h), to be compared stream
 * by stream with pcamv_gpu_annexb_index and header by header with pcamv_gpu_parse_slice_header (pcamv_mvsyntax.h), whose semantics
 * these are on every input, valid or not.  No HIP type.
 *
 * The scan is data-parallel over bytes.  A stream is cut into chunks of SI_CHUNK bytes at addresses that are multiples of 4 (the
 * first chunk is shorter by the stream's misalignment); a wavefront takes one chunk in passes of 256 bytes, one dword per lane, loaded
 * as in pcamv_nal_unescape.h (a whole dword only where all four bytes lie inside the stream).  Byte i is the last of a start code
 * prefix exactly if it is 01 and bytes i - 1, i - 2 are stream bytes and 00: a lane decides that for its four positions from its own
 * dword and the two bytes before it (the lane below; lane 0: the dword before the pass, which for a chunk's first pass is the last
 * dword of the chunk before).  The unit a prefix starts is a slice unit or not by the two bytes behind the prefix alone (si_kind: a
 * header byte 00 is never a slice, and a type-1 unit too short to have its payload byte is followed by 00 or by the end, which reads
 * as "first_mb_in_slice != 0": the same kind either way), so a chunk can count the slice units it starts without knowing where they
 * end.  Twelve ballots -- prefix, slice-starting prefix, non-zero byte, for each of a lane's four positions -- and popcounts below the
 * lane give stream order.
 *
 * Three steps, none of which depends on the order in which wavefronts finish:
 *   si_scan(place = 0)  per chunk: the number of units and of slice units it starts, its last non-zero byte, its last prefix
 *   si_prefix           per stream, one wavefront: the exclusive prefix of the two counts over the stream's chunks, the running
 *                       maximum of the two positions (in place); the stream's totals; the last unit's entry
 *   si_scan(place = 1)  per chunk again: a prefix at i (unit number U) ends unit U - 1, which begins behind the prefix before it and
 *                       ends behind the last non-zero byte before i -- both from the ballots, or from the chunk's carried values, so no
 *                       lane walks a run of zeros -- and the lane writes that unit's entry at its place: U - 1 of all units, or its
 *                       number among the slice units
 * The table takes the first max_units entries; the counts are the full counts.  The longest slice unit written is kept (a maximum:
 * whatever order it is formed in, it is the same number).
 *
 * Nothing outside src[0, len) is read; nothing but the chunk's summary, the first max_units entries of the stream's table and the
 * totals is written.  Results leave through ordinary stores.
 */
#ifndef PCAMV_STREAM_INDEX_H
#define PCAMV_STREAM_INDEX_H
#include "pcamv_nal_unescape.h"

#define SI_CHUNK PCAMV_STREAM_CHUNK     /* bytes of a stream one wavefront scans */
#define SI_PASS 256
#define SI_WIN_DWORDS 65                /* [0] the dword before the pass, [1 .. 64] the pass */
static_assert(SI_CHUNK % SI_PASS == 0 && SI_CHUNK >= SI_PASS, "a chunk is whole passes");

/* per chunk.  After si_scan: what the chunk starts and holds (positions count from the stream's first byte, -1: none).  After
 * si_prefix: the same summed / latest over the chunks before it */
struct SiChunk { long long units, slices, nz, q; };
struct SiWork { uint32_t *win; SiChunk *sc; };          /* LDS of the wave: SI_WIN_DWORDS dwords, 64 summaries */
/* all: every unit, else the selected ones -- the slice units, or with sel == SI_SEL_PSET the units of nal_unit_type 7 and 8, which then
 * are what "slice unit" and `slices` read as throughout (pcamv_param_sets.h) */
#define SI_SEL_PSET 1
struct SiTable { pcamv_unit_t *units; long long max_units; int all; unsigned long long *longest; int sel; };

SP_HD long long si_chunks(const uint8_t *src, long long len) { return len > 0 ? (len + (long long)((uintptr_t)src & 3u) + SI_CHUNK - 1) / SI_CHUNK : 0; }
SP_HD int si_top(uint64_t m) { return 63 - __builtin_clzll(m); }         /* m != 0 */

/* the kind of a unit from its header byte and first payload byte (-1: the stream ends before it) */
SP_HD int si_kind(int h, int p0)
{
    if (h < 0) return PCAMV_UNIT_OTHER;
    const int t = h & 31;
    if (t != 1) return t == 2 || t == 3 || t == 4 ? PCAMV_UNIT_UNSUP : PCAMV_UNIT_OTHER;
    if (p0 < 0 || p0 < 0x80) return PCAMV_UNIT_UNSUP;
    /* slice_type, the ue from bit 6 on: 1 | 01x | 001xx | 0001xxx */
    const int v = p0 & 0x7f;
    const int st = v >= 0x40 ? 0 : v >= 0x20 ? 1 + ((v >> 4) & 1) : v >= 0x10 ? 3 + ((v >> 2) & 3) : v >= 0x08 ? 7 + (v & 7) : 15;
    if (st == 0 || st == 5) return PCAMV_UNIT_PSLICE;
    return st == 2 || st == 7 ? PCAMV_UNIT_OTHER : PCAMV_UNIT_UNSUP;
}
/* is a unit of this header byte and first payload byte one the table selects */
SP_HD int si_selected(const SiTable &T, int h, int p0)
{
    if (T.sel == SI_SEL_PSET) return h >= 0 && ((h & 31) == 7 || (h & 31) == 8);
    return si_kind(h, p0) != PCAMV_UNIT_OTHER;
}
/* the unit src[s, e) into its place of the table: number u among all units, the slices-th slice unit if it is one */
SP_HD void si_emit(const SiTable &T, const uint8_t *src, long long s, long long e, long long u, long long slices_before)
{
    if (e < s) e = s;
    const long long n = e - s;
    const int h = n > 0 ? (int)src[s] : -1, kind = si_kind(h, n > 1 ? (int)src[s + 1] : -1);
    /* (with sel a constant 0 this is the kind just made: the index call's instances read as they did without the other selection) */
    const int picked = T.sel == SI_SEL_PSET ? si_selected(T, h, -1) : kind != PCAMV_UNIT_OTHER;
    const long long at = T.all ? u : picked ? slices_before : -1;
    if (at < 0 || at >= T.max_units) return;
    pcamv_unit_t *o = T.units + at;
    o->off = s; o->len = n; o->nal_header = h; o->kind = kind;
    if (kind != PCAMV_UNIT_OTHER && T.longest) {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicMax(T.longest, (unsigned long long)n);
#else
        if ((unsigned long long)n > *T.longest) *T.longest = (unsigned long long)n;
#endif
    }
}
/* latest position below lane l's byte k that is set in m[0 .. 3] (m[j] bit l': byte j of lane l'), `none` if there is none */
SP_HD long long si_before(const uint64_t m[4], int l, int k, long long pb, long long none)
{
    for (int j = k - 1; j >= 0; j--) if ((m[j] >> l) & 1u) return pb + 4 * l + j;
    const uint64_t below = ((uint64_t)1 << l) - 1u;
    long long best = none;
    for (int j = 0; j < 4; j++) if (m[j] & below) { const long long p = pb + 4 * si_top(m[j] & below) + j; if (p > best) best = p; }
    return best;
}
SP_HD int si_count_before(const uint64_t m[4], int l, int k)
{
    const uint64_t below = ((uint64_t)1 << l) - 1u;
    int n = 0;
    for (int j = 0; j < 4; j++) n += __builtin_popcountll(m[j] & below) + (j < k ? (int)((m[j] >> l) & 1u) : 0);
    return n;
}

/* chunk c of the stream src[0, len).  place == 0: its summary into *C.  place != 0: *C holds what si_prefix made of it, and the units
 * that end at this chunk's prefixes go to the table */
SP_HD void si_scan(const SiWork &W, const uint8_t *src, long long len, long long c, int place, SiChunk *C, const SiTable &T)
{
    const long long a = (long long)((uintptr_t)src & 3u);
    const long long lo = c * SI_CHUNK - a, hi = lo + SI_CHUNK < len ? lo + SI_CHUNK : len;       /* positions lo (may be < 0 in chunk 0) .. hi */
    long long units = 0, slices = 0, nz = -1, q = -1;
    if (place) { units = C->units; slices = C->slices; nz = C->nz; q = C->q; }
    uint32_t tail = SP_UNI(nu_load(src, len, lo - 4));
    for (long long pb = lo; pb < hi; pb += SI_PASS) {
        uint64_t mp[4] = {0, 0, 0, 0}, ms[4] = {0, 0, 0, 0}, mz[4] = {0, 0, 0, 0};
        SP_SYNC();
        SP_LANES(l) {
            W.win[l + 1] = nu_load(src, len, pb + 4 * l);
            if (l == 0) W.win[0] = tail;
        }
        SP_SYNC();
        SP_LANES(l) {
            const uint64_t t = (uint64_t)(W.win[l] >> 16) | (uint64_t)W.win[l + 1] << 16;        /* bytes i0 - 2 .. i0 + 3, i0 = pb + 4 l */
            for (int k = 0; k < 4; k++) {
                const long long i = pb + 4 * l + k;
                const uint32_t b3 = (uint32_t)(t >> (8 * k)) & 0xffffffu;                       /* bytes i - 2, i - 1, i */
                const int in = i >= 0 && i < hi;
                const int pre = in && i >= 2 && b3 == 0x010000u;
                int sl = 0;
                if (pre) sl = si_selected(T, i + 1 < len ? (int)src[i + 1] : -1, i + 2 < len ? (int)src[i + 2] : -1);
                NU_VOTE(mp[k], l, pre); NU_VOTE(ms[k], l, sl); NU_VOTE(mz[k], l, in && (b3 >> 16) != 0);
            }
        }
        tail = SP_UNI(W.win[64]);
        if (place) {
            SP_LANES(l) {
                for (int k = 0; k < 4; k++) {
                    if (!((mp[k] >> l) & 1u)) continue;
                    const long long u = units + si_count_before(mp, l, k);       /* the number of the unit this prefix starts */
                    if (u < 1) continue;
                    const long long pq = si_before(mp, l, k, pb, q), pz = si_before(mz, l, k, pb, nz);
                    /* (slices started so far include unit u - 1 if it is one) */
                    si_emit(T, src, pq + 1, pz + 1, u - 1, slices + si_count_before(ms, l, k) - 1);
                }
            }
        }
        for (int k = 0; k < 4; k++) {
            units += __builtin_popcountll(mp[k]); slices += __builtin_popcountll(ms[k]);
            if (mp[k]) { const long long p = pb + 4 * si_top(mp[k]) + k; if (p > q) q = p; }
            if (mz[k]) { const long long p = pb + 4 * si_top(mz[k]) + k; if (p > nz) nz = p; }
        }
    }
    if (!place) SP_LANES(l) if (l == 0) { C->units = units; C->slices = slices; C->nz = nz; C->q = q; }
}

/* one wavefront per stream, between the two scans: ch[0, n_chunks) from summaries to what lies before each chunk; the stream's
 * totals; the entry of its last unit, which no prefix ends */
SP_HD void si_prefix(const SiWork &W, const uint8_t *src, long long len, SiChunk *ch, long long n_chunks, const SiTable &T, long long *n_units, long long *n_slices)
{
    long long units = 0, slices = 0, nz = -1, q = -1;
    for (long long g = 0; g < n_chunks; g += 64) {
        SP_SYNC();
        SP_LANES(l) {
            const SiChunk none = {0, 0, -1, -1};
            W.sc[l] = g + l < n_chunks ? ch[g + l] : none;
        }
        SP_SYNC();
        SP_LANES(l) {
            SiChunk v = {units, slices, nz, q};
            for (int j = 0; j < l; j++) { v.units += W.sc[j].units; v.slices += W.sc[j].slices; if (W.sc[j].nz > v.nz) v.nz = W.sc[j].nz; if (W.sc[j].q > v.q) v.q = W.sc[j].q; }
            if (g + l < n_chunks) ch[g + l] = v;
        }
        for (int j = 0; j < 64; j++) { units += W.sc[j].units; slices += W.sc[j].slices; if (W.sc[j].nz > nz) nz = W.sc[j].nz; if (W.sc[j].q > q) q = W.sc[j].q; }
    }
    SP_LANES(l) if (l == 0) {
        *n_units = units; *n_slices = slices;
        if (units > 0) si_emit(T, src, q + 1, nz + 1, units - 1, slices - 1);   /* (if it is a slice unit it is the last of them) */
    }
    (void)len;
}

/* ---- the header of a P slice (slice_header(), 7.3.3), one lane per slice */
struct ShBits { const uint8_t *d; long long n_bytes, n_bits, pos; int bad; };
/* the 32 bits from pos on, zeros behind the end */
SP_HD uint32_t sh_peek(const ShBits &b)
{
    const long long at = b.pos >> 3;
    uint64_t w = 0;
    for (int k = 0; k < 5; k++) w = w << 8 | (at + k < b.n_bytes ? (uint64_t)b.d[at + k] : 0u);
    return (uint32_t)(w >> (8 - (int)(b.pos & 7)));
}
SP_HD uint32_t sh_u(ShBits &b, int n)          /* 0 <= n <= 31 */
{
    if (b.bad || n == 0) return 0;
    if (b.pos + n > b.n_bits) { b.bad = 1; return 0; }
    const uint32_t v = sh_peek(b) >> (32 - n);
    b.pos += n;
    return v;
}
SP_HD uint64_t sh_ue(ShBits &b)
{
    if (b.bad) return 0;
    const uint32_t w = sh_peek(b);
    if (!w) { b.bad = 1; return 0; }            /* 32 zeros, or the end among the zeros */
    const int z = __builtin_clz(w);
    if (b.pos + 2 * z + 1 > b.n_bits) { b.bad = 1; return 0; }
    b.pos += z + 1;
    return ((uint64_t)1 << z) - 1u + sh_u(b, z);
}
SP_HD long long sh_se(ShBits &b) { const uint64_t k = sh_ue(b); return k & 1u ? (long long)((k + 1) >> 1) : -(long long)(k >> 1); }

SP_HD int pcamv_slice_header_read(const uint8_t *rbsp, long long len, int nal_header, const pcamv_stream_params_t &P, long long *start_bit, int *slice_qp, int *frame_num)
{
    *start_bit = -1; *slice_qp = -1; *frame_num = -1;
    if (len < 0 || len > (1LL << 40) || P.log2_max_frame_num < 4 || P.log2_max_frame_num > 16 || P.poc_type < 0 || P.poc_type > 2 || P.log2_max_poc_lsb < 4 ||
        P.log2_max_poc_lsb > 16 || P.num_ref_idx_l0_default < 1 || P.num_ref_idx_l0_default > 32 || P.pic_init_qp < 0 || P.pic_init_qp > 51 || P.pps_id < 0 ||
        P.pps_id > 255) return PCAMV_EINVAL;
    if (nal_header < 0 || (nal_header & 31) != 1) return PCAMV_EUNSUP;
    ShBits b = {rbsp, len, 8 * len, 0, 0};
#define SH_READ(v, call) v = (call); if (b.bad) return PCAMV_EINVAL
    uint64_t e; long long s;
    SH_READ(e, sh_ue(b)); if (e) return PCAMV_EUNSUP;                           /* first_mb_in_slice */
    SH_READ(e, sh_ue(b)); if (e != 0 && e != 5) return PCAMV_EUNSUP;            /* slice_type */
    SH_READ(e, sh_ue(b)); if (e != (uint64_t)P.pps_id) return PCAMV_EUNSUP;
    uint32_t fn; SH_READ(fn, sh_u(b, P.log2_max_frame_num));
    if (P.poc_type == 0 || (P.poc_type == 1 && !P.delta_pic_order_always_zero)) {
        if (P.poc_type == 0) { SH_READ(e, sh_u(b, P.log2_max_poc_lsb)); } else { SH_READ(s, sh_se(b)); }
        if (P.pic_order_present) { SH_READ(s, sh_se(b)); }
    }
    if (P.redundant_pic_cnt_present) { SH_READ(e, sh_ue(b)); }
    uint64_t n_ref = (uint64_t)P.num_ref_idx_l0_default;
    SH_READ(e, sh_u(b, 1));
    if (e) { SH_READ(n_ref, sh_ue(b)); n_ref++; }
    if (n_ref != 1) return PCAMV_EUNSUP;
    SH_READ(e, sh_u(b, 1));
    while (e) {                                                                 /* ref_pic_list_reordering: at least two bits a turn */
        uint64_t idc; SH_READ(idc, sh_ue(b));
        if (idc == 3) break;
        if (idc > 3) return PCAMV_EINVAL;
        SH_READ(idc, sh_ue(b));
    }
    if (P.weighted_pred) return PCAMV_EUNSUP;
    if (nal_header & 0x60) { SH_READ(e, sh_u(b, 1)); if (e) return PCAMV_EUNSUP; }
    if (P.entropy_cabac) { SH_READ(e, sh_ue(b)); if (e) return PCAMV_EUNSUP; }
    SH_READ(s, sh_se(b));
    const long long qp = P.pic_init_qp + s;
    if (qp < 0 || qp > 51) return PCAMV_EINVAL;
    if (P.deblocking_filter_control_present) {
        SH_READ(e, sh_ue(b)); if (e > 2) return PCAMV_EINVAL;
        if (e != 1) { SH_READ(s, sh_se(b)); SH_READ(s, sh_se(b)); }
    }
#undef SH_READ
    if (b.pos >= b.n_bits) return PCAMV_EINVAL;
    *start_bit = b.pos; *slice_qp = (int)qp; *frame_num = (int)fn;
    return 0;
}
#endif
