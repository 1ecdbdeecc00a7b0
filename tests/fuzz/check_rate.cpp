/*
 * check_rate.cpp -- TEST-ONLY host build of the control code of k_frame_qp and k_rate_update (csrc/pcamv_rate.h: qprow_dst, qprow_clamp,
 * qprow_take, qprow_put, pcamv_rate_open, pcamv_rate_step), a loop over lanes standing in for the wavefront.  Built with
 * -fsanitize=address,undefined; the row table and every descriptor sit in heap blocks of exactly their size.
 *
 * Rows: for chroma offsets -12 .. 12 and the deadzone pairs of the tests, 52 rows are built as the library builds them (a descriptor
 * through pcamv_frame_set_qp and the two table pointers, qprow_take).  A descriptor filled with a pattern, then patched lane by lane,
 * must equal -- the whole struct, byte for byte -- the same pattern with pcamv_frame_set_qp and the pointers written into it directly,
 * at all 52 QPs; QPs outside 0 .. 51 (negative, 52, INT32_MIN / MAX) must give the row of 0 or 51 and index nothing else (the table
 * ends where row 51 ends); lanes 33 .. 63 must write nothing.
 *
 * The rule: seeded sequences of pictures through pcamv_rate_step, a case per lane as k_rate_update runs it, against a restatement here
 * in 128-bit integers that shares nothing with the header but the parameter struct.
 *
 * usage: check_rate <random sequences> ; prints "rows N ok N" and "sequences N ok N differ 0"
 */
#define PCAMV_HOST_EMU
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pcamv_host_tables.h"
#include "pcamv_rate.h"

static const int DEADZONES[][2] = {{21, 11}, {0, 0}, {32, 32}, {6, 6}, {21, 6}};

static unsigned long long lcg_state = 1;
static unsigned long long rnd() { lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL; return lcg_state >> 11; }

/* the pattern a descriptor holds before the patch: every byte set, so a field the patch leaves alone is told from one it clears */
static void fill(FrameDev *F, unsigned seed) { unsigned char *p = (unsigned char *)F; for (size_t i = 0; i < sizeof(*F); i++) p[i] = (unsigned char)(seed + 31 * i + (i >> 3)); }

static int check_rows(long long *n_out)
{
    long long n = 0, ok = 0;
    int16_t *cost = (int16_t *)malloc(52 * 8);          /* stand-ins for the tables: only their addresses go into the rows */
    uint8_t *cabac = (uint8_t *)malloc(52);
    static const int out_of_range[] = {-1, -2, -52, 52, 53, 64, 1 << 20, INT_MIN, INT_MAX, INT_MIN + 1, INT_MAX - 1};
    for (int mbrd = 0; mbrd < 2; mbrd++)
        for (int off = -12; off <= 12; off++)
            for (size_t z = 0; z < sizeof(DEADZONES) / sizeof(DEADZONES[0]); z++) {
                pcamv_params_t p; memset(&p, 0, sizeof(p));
                p.i_chroma_qp_offset = off; p.i_luma_deadzone[0] = DEADZONES[z][0]; p.i_luma_deadzone[1] = DEADZONES[z][1];
                uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * QPROW_QPS * QPROW_DWORDS);       /* exactly 52 rows */
                for (int qp = 0; qp < QPROW_QPS; qp++) {
                    FrameDev T; memset(&T, 0, sizeof(T)); T.b_mbrd = mbrd;
                    pcamv_frame_set_qp(&T, &p, qp);
                    T.cost_mv = cost + 4 * qp;
                    if (T.b_mbrd) T.cabac_init = cabac + qp;
                    qprow_take(&T, rows + (size_t)qp * QPROW_DWORDS);
                }
                for (int k = 0; k < QPROW_QPS + (int)(sizeof(out_of_range) / sizeof(int)); k++) {
                    const int qp = k < QPROW_QPS ? k : out_of_range[k - QPROW_QPS];
                    const int eff = qp < 0 ? 0 : qp > 51 ? 51 : qp;
                    FrameDev *got = (FrameDev *)malloc(sizeof(FrameDev)), *want = (FrameDev *)malloc(sizeof(FrameDev));
                    fill(got, (unsigned)(k + off)); fill(want, (unsigned)(k + off));
                    pcamv_frame_set_qp(want, &p, eff);
                    want->cost_mv = cost + 4 * eff;
                    if (mbrd) want->cabac_init = cabac + eff; else want->cabac_init = NULL;   /* (a context without RD never had one: the host's descriptor holds NULL) */
                    for (int lane = 0; lane < 64; lane++) qprow_put((uint32_t *)(void *)got, rows, qp, lane);
                    int outside = 0;
                    const int cl = qprow_clamp(qp, &outside);
                    n++;
                    if (!memcmp(got, want, sizeof(FrameDev)) && cl == eff && outside == (qp != eff)) ok++;
                    else if (n - ok < 5) fprintf(stderr, "rows: mbrd %d offset %d deadzones %zu qp %d differ\n", mbrd, off, z, qp);
                    free(got); free(want);
                }
                free(rows);
            }
    free(cost); free(cabac);
    *n_out = n;
    return n == ok;
}

/* ---- the rule restated */
typedef __int128 big;
struct NState { big debt, last_len; long long pictures; int qp, last_d; };
static int naive(const pcamv_rate_params_t &p, NState &s, long long len, int status)
{
    static const long long P[7] = {65536, 73562, 82570, 92682, 104032, 116772, 131072};
    big by = (big)len - s.last_len;
    if (by < 0) by = 0;
    if (by > ((big)1 << 41)) by = (big)1 << 41;
    const big bits = 8 * by, T = p.target_bits, lim = (big)1 << 40;
    s.last_len = len;
    int d = 0;
    if (status) d = p.max_step;
    else {
        s.debt += bits - T;
        if (s.debt > lim) s.debt = lim;
        if (s.debt < -lim) s.debt = -lim;
        big want = T - s.debt / p.window;
        if (want < T / 4) want = T / 4;
        if (want < 1) want = 1;
        for (int k = 0; k <= p.max_step; k++) {
            if (bits >= want && bits * 65536 >= want * P[k]) d = k;
            if (bits < want && want * 65536 >= bits * P[k]) d = -k;
        }
    }
    s.qp += d;
    if (s.qp < p.qp_min) s.qp = p.qp_min;
    if (s.qp > p.qp_max) s.qp = p.qp_max;
    s.last_d = d; s.pictures++;
    return d;
}

int main(int argc, char **argv)
{
    const int n_seq = argc > 1 ? atoi(argv[1]) : 200;
    long long rows = 0;
    const int rows_ok = check_rows(&rows);
    printf("rows %lld ok %lld\n", rows, rows_ok ? rows : -1LL);
    /* sequences: `lanes` cases side by side, as a launch of k_rate_update holds them; states and lengths in blocks of exactly their size */
    static const long long TS[] = {1, 2, 3, 7, 800, 8000, 123457, 1LL << 24, 1LL << 33, 1LL << 40};
    static const int WS[] = {1, 2, 8, 100, 1024};
    int ok = 0, differ = 0;
    for (int q = 0; q < n_seq; q++) {
        const int lanes = 1 + (int)(rnd() % 70);
        std::vector<pcamv_rate_params_t> P((size_t)lanes);
        pcamv_rate_state_t *S = (pcamv_rate_state_t *)malloc(sizeof(pcamv_rate_state_t) * (size_t)lanes);
        long long *len = (long long *)malloc(8 * (size_t)lanes);
        std::vector<NState> N((size_t)lanes);
        int bad = 0;
        for (int i = 0; i < lanes; i++) {
            pcamv_rate_params_t &p = P[(size_t)i];
            memset(&p, 0, sizeof(p));
            p.target_bits = TS[rnd() % 10]; p.qp_min = (int)(rnd() % 40); p.qp_max = p.qp_min + (int)(rnd() % (52 - p.qp_min));
            p.qp_init = p.qp_min + (int)(rnd() % (p.qp_max - p.qp_min + 1)); p.max_step = 1 + (int)(rnd() % 6); p.window = WS[rnd() % 5];
            if (!pcamv_rate_params_ok(&p)) bad = 1;
            len[i] = (long long)(rnd() % (1 << 20));
            pcamv_rate_open(&p, &S[i], len[i]);
            N[(size_t)i] = NState{0, len[i], 0, p.qp_init, 0};
        }
        for (int pic = 0; pic < 300 && !bad; pic++)
            for (int i = 0; i < lanes; i++) {
                const pcamv_rate_params_t &p = P[(size_t)i];
                const unsigned r = (unsigned)(rnd() % 100);
                int status = 0;
                long long add;
                if (r < 5) { status = -3; add = 0; }
                else if (r < 10) add = 0;
                else if (r < 13) add = (long long)(rnd() % (1ULL << 44));
                else if (r < 15) add = -(long long)(rnd() % 1000);
                else { const int sh = (int)(rnd() % 5); add = ((p.target_bits / 8) << sh >> 2) + (long long)(rnd() % 3) + (long long)(rnd() % (p.target_bits / 16 + 1)); }
                len[i] += add;
                if (len[i] < 0) len[i] = 0;
                const int d = pcamv_rate_step(&p, &S[i], len[i], status);
                NState &n = N[(size_t)i];
                const int dn = naive(p, n, len[i], status);
                if (d != dn || S[i].qp != n.qp || (big)S[i].debt != n.debt || (big)S[i].last_len != n.last_len || S[i].pictures != n.pictures || S[i].last_d != n.last_d ||
                    S[i].qp < p.qp_min || S[i].qp > p.qp_max) bad = 1;
            }
        if (bad) { differ++; fprintf(stderr, "sequence %d differs\n", q); } else ok++;
        free(S); free(len);
    }
    printf("sequences %d ok %d differ %d\n", n_seq, ok, differ);
    return rows_ok && !differ ? 0 : 1;
}
