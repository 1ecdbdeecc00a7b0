/* TEST-ONLY: tests/emu/libpcamv_slice_write_cavlc_emu.so -- the device CAVLC slice writer's control code on the CPU (slice_write_cavlc_host.h) */
#include "slice_write_cavlc_host.h"

/* stats (optional): int[3] {clipped level escapes written, bits of the longest block string appended, fold cases} */
extern "C" int swvx_write(const pcamv_params_t *p, int qp, const uint8_t *fy, const uint8_t *fu, const uint8_t *fv, uint8_t *luma4, uint8_t *cu, uint8_t *cv,
                          const pcamv_mb_t *mbs, const int8_t *flip, int n_flip, const uint8_t *hdr_bits, int n_bits, int nal_byte,
                          int as_nal, long long cap, uint8_t *out, long long *len, int *stats)
{
    const SwvHostFrame in = {p, qp, {fy, fu, fv}, luma4, cu, cv, mbs, flip, n_flip};
    uint8_t *buf = (uint8_t *)malloc(cap > 0 ? (size_t)cap : 1);          /* exactly the capacity, wherever the caller's array ends */
    SwvHostStats st = {0, 0, 0};
    const int rc = swv_host_write(in, hdr_bits, n_bits, nal_byte, as_nal, buf, cap, len, &st);
    if (!rc) memcpy(out, buf, (size_t)*len);
    if (stats) { stats[0] = st.n_clip; stats[1] = st.max_block_bits; stats[2] = st.n_fold; }
    free(buf);
    return rc;
}

/* The longest bit string a residual block of `count` positions can have, from the lengths of the table block: the maximum over total,
 * trailing ones, coeff_token class and placement of the zeros of coeff_token + signs + 28 bits per other level + total_zeros +
 * run_before.  dc: the chroma DC tables.  What SWV_BLK_BITS has to hold (16 positions). */
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
extern "C" int swvx_block_bound(int count, int dc)
{
    uint8_t tab[SV_TAB_BYTES];
    if (count < 1 || count > 16 || sv_build_tables(tab)) return -1;
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
extern "C" int swvx_block_bits(void) { return SWV_BLK_BITS; }
