/*
 * pcamv_nal_unescape.h -- the NAL layer undone as control code that compiles for the device and for the host.
 *
 * On the device it is the body of k_nal_to_rbsp (pcamv_slice.hip.h): one wavefront per NAL unit, in front of the two slice parsers.  On
 * the host it is what tests/fuzz/check_nal_unescape.cpp compiles with the scalar form of SP_LANES (pcamv_slice_parse.h), to be compared
 * input by input with pcamv_gpu_nal_to_rbsp (pcamv_mvsyntax.h), whose semantics these are on every input, valid or not: optional Annex B
 * start code (00 00 00 01, else 00 00 01), the header byte (delivered, judged only by its forbidden_zero_bit), then the payload with
 * every 03 that follows two zeros dropped; 00 00 0{0,1,2} and 00 00 03 xx with xx > 03 make the unit PCAMV_EINVAL.  No HIP type.
 *
 * Why the lanes can do it.  The host loop carries a count of zeros, but a zero byte of a valid unit is always kept and every other byte,
 * kept or dropped, sets the count to 0: "zeros >= 2" at payload byte j says no more than that bytes j - 1 and j - 2 are payload bytes
 * and are 00.  So whether byte j is kept, dropped or makes the unit invalid is a function of bytes j - 2 .. j + 1 alone, and a unit is
 * invalid exactly if some byte of it is: the first such byte need not be found.
 *
 * A pass takes 256 source bytes, one dword per lane, dwords aligned as the source address is (a whole-dword load only where all four
 * bytes lie inside the unit, as in sp_refill); the lanes exchange them through `win`.  A lane classifies its four bytes from its own
 * dword, the two bytes before it (the lane below; lane 0: the last dword of the pass before, carried) and the byte after it (the lane
 * above; lane 63 loads that one byte), packs the bytes it keeps and counts them: 0 .. 4.  Three ballots of the count's bits and mbcnt
 * give every lane the number of bytes kept below it, a fourth ballot ORs the lanes' "invalid" into a wave-uniform flag.  The kept bytes
 * go to `out`, a window of the destination in dwords aligned as the destination address is; complete dwords leave with one store per
 * lane, the dword the pass ends in waits at the front of the window for the next pass, and bytes leave singly only at the two ends of
 * the RBSP.  What carries from pass to pass: the output position, the last source dword (its two trailing bytes are looked at), the
 * pending dword.
 *
 * Nothing outside src[0, len) is read where it could matter (the bytes of a dword outside the unit are never loaded); nothing outside
 * dst[0, rbsp_len) is written, and rbsp_len <= len - 1 - (start code).  Results leave through ordinary stores.
 */
#ifndef PCAMV_NAL_UNESCAPE_H
#define PCAMV_NAL_UNESCAPE_H
#include "pcamv_slice_parse.h"

#define NU_PASS 256             /* source bytes of a pass */
#define NU_WIN_DWORDS 66        /* [0] the dword before the pass, [1 .. 64] the pass, [65] the byte behind it */
#define NU_OUT_DWORDS 65        /* 256 bytes kept at most, behind up to 3 bytes of a pending dword */
struct NuWork { uint32_t *win, *out; };         /* LDS of the wave on the device, exact-size heap blocks in the host driver */

#if defined(__HIP_DEVICE_COMPILE__)
/* m: bit l = lane l's p; then the number of lanes below l whose bit is set */
#define NU_VOTE(m, l, p) ((m) = __builtin_amdgcn_ballot_w64(p))
SP_HD int nu_below(uint64_t m, int) { return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
#else
#define NU_VOTE(m, l, p) ((m) |= (uint64_t)((p) ? 1 : 0) << (l))
SP_HD int nu_below(uint64_t m, int l) { return __builtin_popcountll(m & (((uint64_t)1 << l) - 1u)); }
#endif

/* bytes i .. i + 3 of the unit (src + i is dword-aligned), zeros where the unit is not */
SP_HD uint32_t nu_load(const uint8_t *src, long long len, long long i)
{
    uint32_t w = 0;
    if (i >= 0 && i + 3 < len) w = sp_ld32(src + i);
    else for (int k = 0; k < 4; k++) if (i + k >= 0 && i + k < len) w |= (uint32_t)src[i + k] << (8 * k);
    return w;
}

/* src[0, len) -> dst[0, *rbsp_len); *nal_header: the header byte, -1 if the unit has none.  0, or PCAMV_EINVAL with *rbsp_len = -1 (what
 * dst then holds is unspecified, within the same bounds) */
SP_HD int pcamv_nal_unescape(const NuWork &W, const uint8_t *src, long long len, uint8_t *dst, long long *rbsp_len, int *nal_header)
{
    int sc = 0;
    if (len >= 4 && src[0] == 0 && src[1] == 0 && src[2] == 0 && src[3] == 1) sc = 4;
    else if (len >= 3 && src[0] == 0 && src[1] == 0 && src[2] == 1) sc = 3;
    const int hdr = sc < len ? (int)src[sc] : -1;
    int bad = hdr < 0 || (hdr & 0x80);
    const long long p0 = sc + 1;                /* the payload: src[p0, len); the look-behind starts here */
    const long long da = (long long)((uintptr_t)dst & 3u);
    long long opos = 0;                         /* bytes of the RBSP so far */
    uint32_t tail = 0;
    for (long long pb = p0 - (long long)(((uintptr_t)src + (uintptr_t)p0) & 3u); pb < len && !bad; pb += NU_PASS) {
        uint64_t m0 = 0, m1 = 0, m2 = 0, mbad = 0;
        uint32_t kept[SP_SLOTS];
        int cnt[SP_SLOTS];
        SP_SYNC();
        SP_LANES(l) {
            W.win[l + 1] = nu_load(src, len, pb + 4 * l);
            if (l == 0) W.win[0] = tail;
            if (l == 63) W.win[65] = pb + NU_PASS < len ? (uint32_t)src[pb + NU_PASS] : 0u;
        }
        SP_SYNC();
        SP_LANES(l) {
            /* bytes i0 - 2 .. i0 + 4 of the unit, i0 = pb + 4 l, from the low end */
            const uint64_t t = (uint64_t)(W.win[l] >> 16) | (uint64_t)W.win[l + 1] << 16 | (uint64_t)(W.win[l + 2] & 255u) << 48;
            uint32_t kb = 0;
            int c = 0, inv = 0;
            for (int k = 0; k < 4; k++) {
                const long long i = pb + 4 * l + k;
                const uint32_t q = (uint32_t)(t >> (8 * k));            /* bytes i - 2, i - 1, i, i + 1 */
                const uint32_t cur = (q >> 16) & 255u;
                if (i < p0 || i >= len) continue;
                const int z2 = i - 2 >= p0 && (q & 0xffffu) == 0;
                if (z2 && cur == 3) inv |= i + 1 < len && (q >> 24) > 3u;       /* emulation_prevention_three_byte: dropped */
                else if (z2 && cur < 3) inv = 1;
                else kb |= cur << (8 * c++);
            }
            kept[SP_SLOT(l)] = kb; cnt[SP_SLOT(l)] = c;
            NU_VOTE(m0, l, c & 1); NU_VOTE(m1, l, c & 2); NU_VOTE(m2, l, c & 4); NU_VOTE(mbad, l, inv);
        }
        tail = SP_UNI(W.win[64]);
        if (mbad) { bad = 1; break; }
        const int tot = __builtin_popcountll(m0) + 2 * __builtin_popcountll(m1) + 4 * __builtin_popcountll(m2);
        /* the window: dwords of the destination from the one that holds byte opos on; g counts bytes from dst - da */
        const long long g0 = da + opos, gb = g0 & ~3LL, ge = g0 + tot;
        const int last = pb + NU_PASS >= len;
        SP_LANES(l) {
            const int o = (int)(g0 - gb) + nu_below(m0, l) + 2 * nu_below(m1, l) + 4 * nu_below(m2, l);
            for (int k = 0; k < cnt[SP_SLOT(l)]; k++) ((uint8_t *)W.out)[o + k] = (uint8_t)(kept[SP_SLOT(l)] >> (8 * k));
        }
        SP_SYNC();
        SP_LANES(l) {
            for (int d = l; d < NU_OUT_DWORDS; d += 64) {
                const long long g = gb + 4 * d;
                if (g >= ge) continue;
                if (g >= da && g + 4 <= ge) sp_st32(dst + (g - da), W.out[d]);
                else if (g + 4 <= ge || last)           /* the ends of the RBSP; an incomplete dword in between waits for the next pass */
                    for (int k = 0; k < 4; k++) if (g + k >= da && g + k < ge) dst[g + k - da] = (uint8_t)(W.out[d] >> (8 * k));
            }
            /* (window dwords 0 and 64 are lane 0's own) */
            const int pend = (int)(((ge & ~3LL) - gb) >> 2);
            if (l == 0 && pend > 0) W.out[0] = W.out[pend];
        }
        opos += tot;
    }
    SP_LANES(l) if (l == 0) { *rbsp_len = bad ? -1 : opos; *nal_header = hdr; }
    return bad ? PCAMV_EINVAL : 0;
}
#endif
