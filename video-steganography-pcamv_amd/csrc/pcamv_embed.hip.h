/*
 * pcamv_embed.hip.h -- the embedding stage and the receiving side (gfx950), launched by pcamv_gpu.hip only.
 *
 *   k_embed_prepare   cover / cost assembly + MVC adjustment + message (encoder.c:1561-1840)
 *   k_stc_forward / k_stc_backward   syndrome-trellis Viterbi (embed.h:309-548): 1024 states over 1024 / NS threads, then one wave
 *   k_mb_flips        per macroblock: is one of its carriers flipped (what the second pass asks)
 *   k_extract_prepare / k_extract_bits / k_payload_check   the receiving side: carriers of the final motion -> syndrome ->
 *                     packed bytes appended to the context's received stream, and its comparison with the attached payload
 *   k_extract_count / k_extract_chain   k_extract_prepare for a window of frames per context: the carriers of all of them, then the chain
 */
#ifndef PCAMV_EMBED_HIP_H
#define PCAMV_EMBED_HIP_H
#include "pcamv_common.h"
#include "pcamv_prims_gpu.h"
#include "pcamv_logic.h"
#include "stc_mats.h"
#include "pcamv_stc_extract.h"

/* ------------------------------------------------------------------ embedding stage */
struct EmbedDev {
    const pcamv_mb_t *mbs; int n_mb;
    uint8_t *cover, *stego, *message; float *rho; int8_t *flip;
    int *hdr;                 /* [0]=n [1]=m [2]=stc_ok [3]=num_flip [4]=sum(width) [6..7]=(double) sum of rho over the trellis */
    unsigned *cols;           /* [2][STC_MAXW] columns of the two sub-matrices (getMatrix allows widths up to 2^(h-2) = 256, embed.h:286);
                               * cols[2 * STC_MAXW] = shorter, cols[2 * STC_MAXW + 1] = longer */
    unsigned *path;           /* n * 32 words */
    int *rnd;                 /* glibc rand state: r[0..30], f, b */
    long long *lcg;           /* STC column LCG state (embed.h:134) */
    float emrate;
    const uint8_t *user_message; int user_message_len;
    /* payload attached to the context (pcamv_gpu_set_payload*): packed bytes, most significant bit first; NULL = the rand() stream.
     * A frame without a caller's message takes the bits pstate[PST_TX] .. + m and moves that cursor by m on the device. */
    const uint8_t *payload; long long payload_bits;
    long long *pstate;        /* [PST_*] cursors of the payload path (below) */
    int cap;                  /* capacity of the per-carrier arrays */
    int *car_base;            /* [n_mb] index of each macroblock's first carrier (pass 2 finds its flips there) */
    uint8_t *mbflip;          /* [n_mb] 1 = one of the macroblock's carriers is flipped (k_mb_flips, after the backward pass) */
    unsigned *colinfo;        /* per trellis column, what both Viterbi passes need of it in one word: the (shortened)
                               * matrix column as the forward pass uses it [9:0] and as the backward pass does [22:13], cover bit [10], "last column of its message bit" [11], that
                               * message bit [12] */
};

/* (the per-context device words of the payload path, PST_*: pcamv_stc_extract.h) */

/* The receiving side of one frame (k_extract_prepare -> k_extract_bits), and the comparison of the received stream with the payload. */
struct ExtractDev {
    const pcamv_mb_t *mbs; int n_mb, cap;
    const int8_t *flip;       /* flip map in carrier order: the final MV of carrier k is mv_stego where flip[k] == 1 (what
                               * pcamv_gpu_final_mvs applies); NULL: the records hold final MVs already (parsed from a stream) */
    float emrate;
    uint8_t *stego;           /* [cap] LSB(mvx + mvy) of every carrier's final MV */
    uint8_t *bits;            /* [cap] the frame's message bits, one per byte, or NULL */
    int *hdr;                 /* [0]=n [1]=m [2]=sub-matrices built [6..7]=(long long) bit offset of the frame in the received stream */
    unsigned *cols;           /* [2][STC_MAXW] */
    long long *pstate;
    unsigned *rx; long long rx_cap_bits;          /* received stream: packed, zeroed when reserved / reset; NULL = nothing is appended */
    const uint8_t *payload; long long payload_bits;
    int *slice_status;        /* records parsed from a slice on the device (k_parse_pslice): the parser's return code; != 0: the frame
                               * appends nothing, cursor and column generator stay as they are.  NULL: not from a slice */
};

__device__ __forceinline__ int dev_is01(int d) { return d == 0 || d == 1; }

__device__ int dev_glibc_rand(int *st)
{
    int f = st[31], b = st[32];
    unsigned v = (unsigned)st[f] + (unsigned)st[b];
    st[f] = (int)v;
    if (++f >= 31) f = 0;
    if (++b >= 31) b = 0;
    st[31] = f; st[32] = b;
    return (int)((v >> 1) & 0x7fffffff);
}
/* (pcamv_stc_extract.h: the builder the host check of the receive-side chain compiles too) */
__device__ __forceinline__ int dev_stc_matrix(int width, int height, unsigned *cols, long long *lcg) { return pcamv_stc_matrix(pcamv_stc_mats_dev, width, height, cols, lcg); }

/* Carriers of a frame's records in embedding order (encoder.c:1566-1647), for a workgroup of 1024: every thread takes a run of
 * macroblocks [*lo, *hi), and gets the index of its first carrier in *base; returns the frame's carrier count.  Sender and
 * receiver share the walk; they differ in what tells a carrying macroblock: the record's own flag (sender), or -- all a decoder
 * knows -- that the macroblock is coded (DECODER: i_type != P_SKIP; the same set, encoder.c:1566). */
template <bool DECODER>
__device__ __forceinline__ int dev_carrier_scan(const pcamv_mb_t *__restrict__ mbs, int n_mb, int *s_cnt, int *lo_out, int *hi_out, int *base_out)
{
    const int t = threadIdx.x;
    const int chunk = (n_mb + 1023) / 1024;
    const int lo = t * chunk, hi = min(n_mb, lo + chunk);
    int cnt = 0, slots[16];
    for (int xy = lo; xy < hi; xy++) {
        const pcamv_mb_t *mb = &mbs[xy];
        cnt += carrier_slots(mb->i_type, mb->i_partition, mb->i_sub_partition, DECODER ? mb->i_type != PCAMV_P_SKIP : mb->used, slots);
    }
    s_cnt[t] = cnt;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {          /* inclusive Hillis-Steele scan */
        int v = t >= off ? s_cnt[t - off] : 0;
        __syncthreads();
        s_cnt[t] += v;
        __syncthreads();
    }
    *lo_out = lo; *hi_out = hi; *base_out = s_cnt[t] - cnt;
    return s_cnt[1023];
}

static __global__ void __launch_bounds__(1024) k_embed_prepare(const EmbedDev *__restrict__ Es)
{
    const EmbedDev E = Es[blockIdx.x];
    __shared__ int s_cnt[1024];
    const int t = threadIdx.x;
    int lo, hi, base, slots[16];
    const int n = dev_carrier_scan<false>(E.mbs, E.n_mb, s_cnt, &lo, &hi, &base);
    const float mvc_c1 = 2, mvc_c2 = 0.7f;
    for (int xy = lo; xy < hi; xy++) {
        const pcamv_mb_t *mb = &E.mbs[xy];
        int k = carrier_slots(mb->i_type, mb->i_partition, mb->i_sub_partition, mb->used, slots);
        E.car_base[xy] = base;
        if (!k) continue;
        float rho[16];
        for (int i = 0; i < k; i++) {
            E.cover[base + i] = (uint8_t)((mb->mv[slots[i]][0] + mb->mv[slots[i]][1]) & 1);
            rho[i] = (float)mb->inter_stego_cost[slots[i]];
        }
#define MVD(a, b, c) iabs(mb->mv[a][c] - mb->mv[b][c])
        if (mb->i_type == PCAMV_P_8x8) {
            const uint8_t *sp = mb->i_sub_partition;
            int len = 0;
            if (sp[0] == PCAMV_D_L0_8x8 && sp[1] == PCAMV_D_L0_8x8 && sp[2] == PCAMV_D_L0_8x8 && sp[3] == PCAMV_D_L0_8x8) {
                int c = dev_is01(MVD(0, 4, 0)) + dev_is01(MVD(4, 12, 0)) + dev_is01(MVD(12, 8, 0)) + dev_is01(MVD(8, 0, 0)) +
                        dev_is01(MVD(0, 4, 1)) + dev_is01(MVD(4, 12, 1)) + dev_is01(MVD(12, 8, 1)) + dev_is01(MVD(8, 0, 1));
                float fac = __fadd_rn(__fmul_rn(mvc_c2, (float)c), 1.0f);
                for (int j = 0; j < 4; j++) rho[j] = __fmul_rn(rho[j], fac);
            }
            for (int i = 0; i < 4; i++) {
                if (sp[i] == PCAMV_D_L0_8x8) len += 1;
                else if (sp[i] == PCAMV_D_L0_4x8 || sp[i] == PCAMV_D_L0_8x4) {
                    int b = sp[i] == PCAMV_D_L0_4x8 ? 4 * i + 1 : 4 * i + 2;
                    if (MVD(4 * i, b, 0) + MVD(4 * i, b, 1) < 2) { rho[len] = __fmul_rn(rho[len], mvc_c1); rho[len + 1] = __fmul_rn(rho[len + 1], mvc_c1); }
                    len += 2;
                } else {
                    int q = 4 * i;
                    int c = dev_is01(MVD(q, q + 1, 0)) + dev_is01(MVD(q + 1, q + 3, 0)) + dev_is01(MVD(q + 2, q + 3, 0)) + dev_is01(MVD(q, q + 2, 0)) +
                            dev_is01(MVD(q, q + 1, 1)) + dev_is01(MVD(q + 1, q + 3, 1)) + dev_is01(MVD(q + 2, q + 3, 1)) + dev_is01(MVD(q, q + 2, 1));
                    float fac = __fadd_rn(__fmul_rn(mvc_c2, (float)c), 1.0f);
                    for (int j = 0; j < 4; j++) rho[len + j] = __fmul_rn(rho[len + j], fac);
                    len += 4;
                }
            }
        } else if (mb->i_partition != PCAMV_D_16x16) {
            int b = mb->i_partition == PCAMV_D_8x16 ? 4 : 8;
            if (MVD(0, b, 0) + MVD(0, b, 1) < 2) { rho[0] = __fmul_rn(rho[0], mvc_c1); rho[1] = __fmul_rn(rho[1], mvc_c1); }
        }
#undef MVD
        for (int i = 0; i < k; i++) E.rho[base + i] = rho[i];
        base += k;
    }
    for (int i = t; i < E.cap; i += 1024) { E.stego[i] = 0; E.flip[i] = 0; }
    /* ---- message, sub-matrix schedule (embed.h:340-393), per-column constants ----
     * The schedule "take the longer sub-matrix while the columns used so far stay <= (i + 1) * invalpha + 0.5"
     * has the closed form  columns before message bit i = floor(i * invalpha + 0.5)  (each step adds floor or ceil
     * of invalpha, and the rule picks the one that lands on the next floor; tests/test_stc_schedule.py checks the
     * two agree in the same double arithmetic), so message bits are independent and only the message itself (a
     * lagged-Fibonacci generator) and the sum of rho stay serial, one wave each. */
    __shared__ unsigned s_rnd[64];
    __shared__ unsigned s_cols[2 * STC_MAXW];
    __shared__ int s_ok;
    const int m = pcamv_stc_frame_bits(E.emrate, n);
    const bool sched = m > 0 && m <= n;
    const double invalpha = sched ? (double)n / m : 0.0;
    const int shorter = (int)floor(invalpha), longer = (int)ceil(invalpha);
#define STC_BEFORE(i) ((i) == 0 ? 0 : (int)floor((i) * invalpha + 0.5))
    const int nproc = sched ? STC_BEFORE(m) : 0;
    if (t == 64) {
        /* (built in LDS: the random-column generator compares every new column with all earlier ones, a serial walk
         * that should not go through global memory) */
        const int ok = sched && dev_stc_matrix(shorter, 10, s_cols, E.lcg) && dev_stc_matrix(longer, 10, s_cols + STC_MAXW, E.lcg);
        if (ok) {
            for (int k = 0; k < shorter; k++) E.cols[k] = s_cols[k];
            for (int k = 0; k < longer; k++) E.cols[STC_MAXW + k] = s_cols[STC_MAXW + k];
            E.cols[2 * STC_MAXW] = shorter; E.cols[2 * STC_MAXW + 1] = longer;
        }
        E.hdr[0] = n; E.hdr[1] = m; E.hdr[3] = 0;
        E.hdr[4] = ok ? nproc : 0; E.hdr[2] = ok ? -1 : 0;          /* -1: schedule valid, Viterbi pending */
        s_ok = ok;
    }
    if (t < 64) {
        if (E.user_message) {
            for (int i = t; i < imin(m, E.cap); i += 64) E.message[i] = i < E.user_message_len ? E.user_message[i] : 0;     /* m > n (> cap) fails in stc_embed like the reference's; never write past the arrays */
        } else if (!E.payload) {
            /* glibc TYPE_3 rand(): x[k] = x[k-31] + x[k-3], output x[k] >> 1.  Three outputs are independent of each
             * other, so lanes 0..2 make three per round on a 64-entry ring in LDS.  The stored state is a 31-entry
             * ring with the oldest value at st[31] (f): x[-31 + j] = st[(f + j) % 31]. */
            const int f = E.rnd[31];
            if (t < 31) s_rnd[33 + t] = (unsigned)E.rnd[(f + t) % 31];         /* x[-31 + t] at ring position (-31 + t) & 63 */
            PCAMV_WAVE_SYNC();
            for (int k0 = 0; k0 < m; k0 += 3) {
                const int k = k0 + t;
                if (t < 3 && k < m) {
                    const unsigned v = s_rnd[(k - 31) & 63] + s_rnd[(k - 3) & 63];
                    s_rnd[k & 63] = v;
                    if (k < E.cap) E.message[k] = (uint8_t)(v >> 1 & 1);      /* the stream advances by m whatever the capacity */
                }
                PCAMV_WAVE_SYNC();
            }
            if (t < 31) E.rnd[(f + m + t) % 31] = (int)s_rnd[(m - 31 + t) & 63];
            if (t == 0) { E.rnd[31] = (f + m) % 31; E.rnd[32] = (E.rnd[32] + m) % 31; }
        }
    }
    /* an attached payload: bit cursor + i of it to message bit i, zeros past its end; one bit per lane, the whole workgroup (nothing
     * serial to wait for, and the rand() state does not move).  The cursor advances by m whatever becomes of the frame -- the
     * rule of the rand() stream -- so a frame whose embedding fails costs its own m bits and nothing after them. */
    const bool from_payload = !E.user_message && E.payload;
    const long long cursor = from_payload ? E.pstate[PST_TX] : 0;
    if (from_payload)
        for (int i = t; i < imin(m, E.cap); i += 1024) E.message[i] = cursor + i < E.payload_bits ? (uint8_t)pcamv_packed_bit(E.payload, cursor + i) : 0;
    __syncthreads();
    if (from_payload && t == 0) E.pstate[PST_TX] = cursor + m;          /* (every thread has read the cursor: the barrier above) */
    if (!s_ok) return;
    for (int i = t; i < m; i += 1024) {
        const int start = STC_BEFORE(i);
        const int which = (double)(start + longer) <= (i + 1) * invalpha + 0.5, width = which ? longer : shorter;
        /* shortened columns near the end of the message.  The forward pass drops one row after every message bit i with
         * m - i <= 10 (embed.h:462), the backward pass adds one row back per such bit from the end (embed.h:523): the same
         * mask when m >= 10, not for shorter messages -- the reference's own arithmetic, kept (its stego then does not
         * carry the message) */
        const int left = m - i, drops = imax(0, i - imax(0, m - 10));
        const unsigned fmask = 1023u >> drops, bmask = left >= 10 ? 1023u : (1u << left) - 1, msg = E.message[i] ? 4096u : 0u;
        for (int k = 0; k < width; k++) {
            const unsigned col = s_cols[which * STC_MAXW + k];
            E.colinfo[start + k] = (col & fmask) | (E.cover[start + k] ? 1024u : 0u) | (k == width - 1 ? 2048u : 0u) | msg | (col & bmask) << 13;
        }
    }
#undef STC_BEFORE
    if (t >= 960) {         /* the price of flipping everything, summed in column order like embed.h:448 (the Viterbi's
                             * failure test compares against it): one wave, 64 loads at a time, serial adds */
        const int l = t - 960;
        double total = 0;
        for (int b0 = 0; b0 < nproc; b0 += 64) {        /* columns past the end add +0.0: no effect on a sum of non-negatives */
            const double v = b0 + l < nproc ? (double)E.rho[b0 + l] : 0.0;
            const int lo = __double2loint(v), hi = __double2hiint(v);
#pragma unroll
            for (int i = 0; i < 64; i++) total += __hiloint2double(__builtin_amdgcn_readlane(hi, i), __builtin_amdgcn_readlane(lo, i));
        }
        if (l == 0) *(double *)(E.hdr + 6) = total;
    }
}

/* forward Viterbi over the 1024 trellis states: new[s] = min(p[s] + c_stay, p[s^col] + c_flip), path bit set
 * when the flip branch is <= (embed.h:439-467 evaluated per state; ties and infinities behave identically
 * because both formulations add and compare the same two floats).  The trellis columns are a serial chain with
 * one workgroup barrier each, and what the kernel costs is the time of one link of that chain, so:
 *   - 1024 / NS threads x NS states (s = t + NT j): the per-column bookkeeping is paid once per wave, and a
 *     thread's own p[s] stays in registers;
 *   - the column's constants are fetched one column ahead;
 *   - the fold at the end of a message bit (keep the states whose LSB is that bit, embed.h:469-480) is computed
 *     with the bit's last column instead of in a step of its own;
 *   - the sum of all rho the result is tested against (embed.h:448) is made by k_embed_prepare;
 *   - the barrier waits for LDS traffic only -- __syncthreads() would also drain the path-row stores (s_waitcnt
 *     vmcnt(0)), which nothing in this kernel reads back. */
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
template <int NS>
__global__ void __launch_bounds__(1024 / NS) k_stc_forward(const EmbedDev *__restrict__ Es)
{
    constexpr int NT = 1024 / NS, LOG_NT = NS == 1 ? 10 : NS == 2 ? 9 : 8;
    const EmbedDev E = Es[blockIdx.x];
    __shared__ float s_p[2][1024];
    __shared__ float s_rho[2][256];
    __shared__ unsigned s_info[2][256];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (E.hdr[2] != -1) return;
    const int nproc = E.hdr[4];
    typedef __attribute__((address_space(1))) unsigned long long *gp64w;
    gp64w path = (gp64w)E.path;                         /* global_store, not flat: a flat store also counts on lgkmcnt */
    const float inf = __int_as_float(0x7F800000);
    int cur = 0;
    float p[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) { p[j] = t + j == 0 ? 0.0f : inf; s_p[0][t + NT * j] = p[j]; }
    if (t < 256 && t < nproc) { s_rho[0][t] = E.rho[t]; s_info[0][t] = E.colinfo[t]; }
    __syncthreads();
    unsigned info = s_info[0][0];
    float r = s_rho[0][0];
    for (int index = 0; index < nproc; index++) {
        const int c = index & 255, buf = index >> 8 & 1;
        if (c == 0 && t < 256) {                        /* next 256 columns' constants into the other buffer */
            const int j = index + 256 + t;
            if (j < nproc) { s_rho[buf ^ 1][t] = E.rho[j]; s_info[buf ^ 1][t] = E.colinfo[j]; }
        }
        const int nx = index + 1;
        const unsigned info_n = s_info[nx >> 8 & 1][nx & 255];
        const float r_n = s_rho[nx >> 8 & 1][nx & 255];
        const unsigned column = info & 1023u, xlo = (unsigned)t ^ (column & (NT - 1)), chi = column >> LOG_NT;
        const float c1 = info & 1024u ? r : 0.0f, c2 = info & 1024u ? 0.0f : r;
        float nv[NS];
        unsigned long long bal = 0;
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const float stay = __fadd_rn(p[j], c1), flp = __fadd_rn(s_p[cur][xlo + (((unsigned)j ^ chi) << LOG_NT)], c2);
            const bool bit = flp <= stay;
            nv[j] = bit ? flp : stay;
            const unsigned long long b = __ballot(bit);                 /* states NT j + 64 wv ..: 64-bit word (NT / 64) j + wv of the path row */
            bal = lane == j ? b : bal;
        }
        if (lane < NS) path[(size_t)index * 16 + (NT / 64) * lane + wv] = bal;
        if (info & 2048u) {                             /* last column of a message bit: state s continues as 2s + bit */
#pragma unroll
            for (int j = 0; j < NS; j++) {
                if (NT * j >= 512) { nv[j] = inf; continue; }
                const unsigned sj = t + NT * j, t2 = (2u * sj + (info >> 12 & 1)) & 1023u;
                const float stay2 = __fadd_rn(s_p[cur][t2], c1), flp2 = __fadd_rn(s_p[cur][t2 ^ column], c2);
                nv[j] = sj < 512 ? (flp2 <= stay2 ? flp2 : stay2) : inf;
            }
        }
#pragma unroll
        for (int j = 0; j < NS; j++) { p[j] = nv[j]; s_p[cur ^ 1][t + NT * j] = nv[j]; }
        cur ^= 1;
        LDS_BARRIER();
        info = info_n; r = r_n;
    }
    if (t == 0) {
        const double totalprice = p[0], total = *(const double *)(E.hdr + 6);
        E.hdr[2] = (totalprice >= total) ? 0 : -2;     /* -2: forward ok, backward pending */
    }
}

/* backward walk (embed.h:483-520): one wave, 64 trellis columns per round.  Their path rows sit in registers,
 * word w of every row in lane w, so the serial walk is scalar code around one v_readlane per column; the
 * column's constants (colinfo) come from the lane of the same number.  The walk's state is wave-uniform: the
 * compiler keeps it in SGPRs. */
static __global__ void __launch_bounds__(64) k_stc_backward(const EmbedDev *__restrict__ Es)
{
    const EmbedDev E = Es[blockIdx.x];
    const int lane = threadIdx.x;
    const int n = E.hdr[0];
    int nf = 0, done_upto = 0;             /* elements [0, done_upto) got their stego bit here */
    if (E.hdr[2] == -2) {
        int index = E.hdr[4] - 1;
        done_upto = E.hdr[4];
        unsigned state = 0;
        while (index >= 0) {
            const int base = index >= 63 ? index - 63 : 0, cnt = index - base + 1;
            unsigned row[64];
#pragma unroll
            for (int e = 0; e < 64; e++) row[e] = (e < cnt && lane < 32) ? E.path[(size_t)(base + e) * 32 + lane] : 0u;
            const unsigned info = lane < cnt ? E.colinfo[base + lane] : 0u;
            unsigned long long out = 0;
#pragma unroll
            for (int e = 63; e >= 0; e--) {
                if (e < cnt) {
                    const unsigned inf = __builtin_amdgcn_readlane(info, e);
                    if (inf & 2048u) state = (state << 1) | (inf >> 12 & 1);
                    const unsigned word = __builtin_amdgcn_readlane(row[e], (state >> 5) & 31);
                    if (word >> (state & 31) & 1) { out |= 1ull << e; state ^= inf >> 13 & 1023u; }
                }
            }
            if (lane < cnt) {       /* stego bit and flip map (encoder.c:1848-1855) of this chunk */
                int st = (int)(out >> lane & 1), f = (int)(info >> 10 & 1) ^ st;
                E.stego[base + lane] = (uint8_t)st; E.flip[base + lane] = (int8_t)f; nf += f;
            }
            index = base - 1;
        }
    }
    /* everything not reached by the Viterbi (failure, m == 0, tail) keeps stego = 0: flip = cover */
    for (int i = done_upto + lane; i < n; i += 64) { int f = E.cover[i]; E.flip[i] = (int8_t)f; nf += f; }
    nf = wave_sum_all(nf);
    if (lane == 0) { E.hdr[3] = nf; E.hdr[2] = E.hdr[2] == -2 ? 1 : 0; }
}
/* per macroblock: is any of its carriers flipped?  The second pass asks this with the macroblock's record instead of looking at the
 * carriers' flags after it (one memory round trip less on its path; 7 of 8 macroblocks at half a bit per carrier have none) */
static __global__ void __launch_bounds__(256) k_mb_flips(const EmbedDev *__restrict__ Es)
{
    const EmbedDev &E = Es[blockIdx.y];
    const int xy = (int)(blockIdx.x * 256 + threadIdx.x);
    if (xy >= E.n_mb) return;
    const int n = E.hdr[0], a = E.car_base[xy], b = xy + 1 < E.n_mb ? E.car_base[xy + 1] : n;
    int any = 0;
    for (int i = a; i < b && i < n; i++) any |= E.flip[i] == 1;
    E.mbflip[xy] = (uint8_t)any;
}
/* ------------------------------------------------------------------ receiving side
 * (the reference has no extractor; this is the library's own, pcamv_gpu_stc_extract_lcg, on the device)
 * k_extract_prepare, one workgroup per frame: the carriers of the frame as a decoder finds them, the LSB of each one's final MV,
 * then on one thread what chains from frame to frame (pcamv_extract_chain_slot, pcamv_stc_extract.h): the frame's n and m, the two
 * sub-matrices from the receiver's own column generator, and the frame's place in the received stream.
 * A window of frames per context (k_extract_count, k_extract_chain) splits the two: the carriers of every frame of the window at once,
 * then the chain over a context's frames in order. */
/* the parallel part, a workgroup of 1024: X.stego filled, the frame's carrier count returned to every thread */
__device__ __forceinline__ int dev_extract_carriers(const ExtractDev &X, int *s_cnt)
{
    int lo, hi, base, slots[16];
    const int n = dev_carrier_scan<true>(X.mbs, X.n_mb, s_cnt, &lo, &hi, &base);
    for (int xy = lo; xy < hi; xy++) {
        const pcamv_mb_t *mb = &X.mbs[xy];
        const int k = carrier_slots(mb->i_type, mb->i_partition, mb->i_sub_partition, mb->i_type != PCAMV_P_SKIP, slots);
        for (int i = 0; i < k && base + i < X.cap; i++) {
            const int16_t *mv = X.flip && X.flip[base + i] == 1 ? mb->mv_stego[slots[i]] : mb->mv[slots[i]];
            X.stego[base + i] = (uint8_t)((mv[0] + mv[1]) & 1);
        }
        base += k;
    }
    return n;
}
static __global__ void __launch_bounds__(1024) k_extract_prepare(const ExtractDev *__restrict__ Xs)
{
    const ExtractDev X = Xs[blockIdx.x];
    __shared__ int s_cnt[1024];
    __shared__ unsigned s_cols[2 * STC_MAXW];
    const int t = threadIdx.x;
    if (X.slice_status && *X.slice_status) {            /* (the whole workgroup: no barrier was reached) the slice did not parse: no bits */
        if (t == 64) pcamv_extract_chain_slot(pcamv_stc_mats_dev, X.emrate, 1, X.rx != NULL, X.rx_cap_bits, X.hdr, s_cols, X.cols, X.pstate);
        return;
    }
    const int n = dev_extract_carriers(X, s_cnt);
    if (t == 64) {
        X.hdr[0] = n;
        pcamv_extract_chain_slot(pcamv_stc_mats_dev, X.emrate, 0, X.rx != NULL, X.rx_cap_bits, X.hdr, s_cols, X.cols, X.pstate);
    }
}
/* the window's first half, one workgroup per (context, slot): the slot's carriers and hdr[0] = n; a slot whose slice did not parse
 * (or that took no unit) gets n = 0 and nothing else */
static __global__ void __launch_bounds__(1024) k_extract_count(const ExtractDev *__restrict__ Xs)
{
    const ExtractDev X = Xs[blockIdx.x];
    __shared__ int s_cnt[1024];
    if (X.slice_status && *X.slice_status) {            /* (the whole workgroup: no barrier was reached) */
        if (threadIdx.x == 64) X.hdr[0] = 0;
        return;
    }
    const int n = dev_extract_carriers(X, s_cnt);
    if (threadIdx.x == 64) X.hdr[0] = n;
}
/* the window's second half, one lane per context: the k slots of context i (Xs[i * k .. + k)) in slot order through
 * pcamv_extract_chain_slot -- per slot a table copy or a short walk of the generator, so 64 contexts share a wave and nothing here
 * is lane-parallel.  The columns are built where k_extract_bits reads them (a slot's own cols: LDS for 64 lanes' worth would be 128 KB) */
static __global__ void __launch_bounds__(64) k_extract_chain(const ExtractDev *__restrict__ Xs, int n, int k)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    for (int w = 0; w < k; w++) {
        const ExtractDev &X = Xs[(long long)i * k + w];
        pcamv_extract_chain_slot(pcamv_stc_mats_dev, X.emrate, X.slice_status ? *X.slice_status : 0, X.rx != NULL, X.rx_cap_bits, X.hdr, X.cols, X.cols, X.pstate);
    }
}

/* k_extract_bits: one thread per message bit (pcamv_stc_extract_bit, shared with the host), the sub-matrices in LDS, the stego
 * columns a workgroup's 256 bits reach staged through LDS when they fit (265 blocks of up to EXTRACT_WIN / 265 = 30 columns; wider
 * sub-matrices mean few message bits, those read global memory).  Threads are laid over the received stream from a 64-bit
 * boundary below the frame's first bit, so a wave's ballot is eight whole bytes of the stream: reversed to most-significant-bit
 * first and OR-ed in as two words (a frame's first and last byte may be shared with its neighbours'; the stream is zeroed when
 * reserved).  Bits at or beyond the reserved capacity are dropped here, never written. */
#define EXTRACT_WIN 8192
static __global__ void __launch_bounds__(256) k_extract_bits(const ExtractDev *__restrict__ Xs)
{
    const ExtractDev X = Xs[blockIdx.y];
    __shared__ unsigned s_cols[2 * STC_MAXW];
    __shared__ uint8_t s_win[EXTRACT_WIN];
    const int t = threadIdx.x, lane = t & 63;
    const int n = X.hdr[0], ok = X.hdr[2];
    const int m = imin(X.hdr[1], X.cap);                /* (ok: m <= n <= cap; else only the zeros of `bits` are left to write) */
    if (!ok) {
        if (X.bits) for (int j = blockIdx.x * 256 + t; j < m; j += gridDim.x * 256) X.bits[j] = 0;
        return;
    }
    const long long at = *(const long long *)(X.hdr + 6);
    const int lead = (int)(at & 63);                    /* positions between the 64-bit boundary and the frame's first bit */
    const long long pos0 = at - lead;
    const double invalpha = (double)n / m;
    const int shorter = (int)floor(invalpha), longer = (int)ceil(invalpha);
    for (int k = t; k < shorter; k += 256) s_cols[k] = X.cols[k];
    for (int k = t; k < longer; k += 256) s_cols[STC_MAXW + k] = X.cols[STC_MAXW + k];
    for (int g0 = blockIdx.x * 256; g0 < lead + m; g0 += gridDim.x * 256) {        /* (workgroup-uniform: barriers inside) */
        const int j = g0 + t - lead;
        int wlo, whi;
        pcamv_stc_window(imax(g0 - lead, 0), g0 - lead + 256, n, m, invalpha, PCAMV_STC_HEIGHT, &wlo, &whi);
        const bool staged = whi - wlo <= EXTRACT_WIN;
        __syncthreads();                                /* s_cols written / the last round's window read */
        if (staged) {
            for (int k = t; k < whi - wlo; k += 256) s_win[k] = X.stego[wlo + k];
            __syncthreads();
        }
        const unsigned bit = j >= 0 && j < m ? pcamv_stc_extract_bit(staged ? s_win : X.stego, staged ? wlo : 0, n, m, invalpha, shorter, longer,
                                                                      s_cols, s_cols + STC_MAXW, PCAMV_STC_HEIGHT, j) : 0u;
        if (X.bits && j >= 0 && j < m) X.bits[j] = (uint8_t)bit;
        const long long pos = pos0 + g0 + t;
        const unsigned long long bal = __ballot(bit && X.rx && pos < X.rx_cap_bits);
        if (lane < 2) {
            const unsigned w = __builtin_bswap32(__brev((unsigned)(bal >> (32 * lane))));          /* bit-reversed inside every byte */
            const long long word = ((pos - lane) >> 5) + lane;
            if (w && word < ((X.rx_cap_bits + 31) >> 5)) atomicOr(&X.rx[word], w);
        }
    }
}

/* bits in which a context's received stream differs from its attached payload (the BER numerator), over the bits received so far;
 * payload bits past its end count as zeros.  One workgroup per context. */
static __global__ void __launch_bounds__(256) k_payload_check(const ExtractDev *__restrict__ Xs, long long *__restrict__ out)
{
    const ExtractDev X = Xs[blockIdx.x];
    __shared__ int s_sum[4];
    const int t = threadIdx.x;
    long long got = X.rx ? X.pstate[PST_RX] : 0;
    if (got > X.rx_cap_bits) got = X.rx_cap_bits;
    const uint8_t *rx = (const uint8_t *)X.rx;
    const long long nbytes = (got + 7) >> 3, pbytes = X.payload ? (X.payload_bits + 7) >> 3 : 0;
    int diff = 0;
    for (long long b = t; b < nbytes; b += 256) {
        unsigned p = b < pbytes ? X.payload[b] : 0u;
        if (b == pbytes - 1 && (X.payload_bits & 7)) p &= 0xff00u >> (X.payload_bits & 7);         /* what the caller's last byte holds beyond the payload */
        unsigned d = rx[b] ^ p;
        if (b == nbytes - 1 && (got & 7)) d &= 0xff00u >> (got & 7);
        diff += __popc(d & 0xffu);
    }
    diff = wave_sum_all(diff);
    if ((t & 63) == 0) s_sum[t >> 6] = diff;
    __syncthreads();
    if (t == 0) out[blockIdx.x] = (long long)s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}
#endif
