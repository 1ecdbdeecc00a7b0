/*
 * pcamv_stc_extract.h -- the receiving side of the syndrome-trellis code, one message bit at a time.
 *
 * Compiles for the device (k_extract_prepare / k_extract_chain / k_extract_chain_message / k_extract_bits, and the message length and matrix builder
 * k_embed_prepare shares with them), for the host side of the library (the column generator of pcamv_gpu_stc_extract_lcg) and for
 * plain C++ test programs (tests/emu/stc_extract_driver.cpp, tests/fuzz/check_extract_window.cpp): no HIP type, no table of its own.
 *
 * The extractor of embed.h:340-393 is H * y over GF(2) with H made of two sub-matrices laid along the diagonal: message bit i owns
 * `width(i)` columns starting at column before(i) of the stego vector, and column k of that block reaches the message bits
 * i .. i + height - 1 with the bits of cols_i[k].  With the closed-form schedule before(i) = floor(i * invalpha + 0.5)
 * (k_embed_prepare, tests/test_stc_schedule.py) message bit j needs nothing but the blocks j - (height - 1) .. j:
 *
 *     message[j] = XOR over i = j - (height - 1) .. j, k < width(i) of  stego[before(i) + k] & (cols_i[k] >> (j - i))
 *
 * so every message bit is independent of the others.
 */
#ifndef PCAMV_STC_EXTRACT_H
#define PCAMV_STC_EXTRACT_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PCAMV_HD __host__ __device__ static inline
#else
#define PCAMV_HD static inline
#endif

#ifndef STC_MAXW
#define STC_MAXW 256          /* getMatrix allows widths up to 2^(h-2) = 256 at height 10 (embed.h:286) */
#endif
#define PCAMV_STC_HEIGHT 10   /* the matrix height the fork embeds with (encoder.c:1843) */

/* message bits of a frame with n carriers (encoder.c:1828-1836): emrate <= 1 is bits per motion vector, in single precision with
 * one rounding (the embedding kernel and the receiver must agree to the bit), emrate > 1 is bits per frame */
PCAMV_HD int pcamv_stc_frame_bits(float emrate, int n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int m = emrate > 1.0f ? (int)emrate : (int)__fmul_rn(emrate, (float)n);
#else
    int m = emrate > 1.0f ? (int)emrate : (int)(emrate * (float)n);
#endif
    return m < 0 ? 0 : m;
}

/* stego columns in front of message bit i */
PCAMV_HD int pcamv_stc_before(int i, double invalpha) { return i == 0 ? 0 : (int)floor(i * invalpha + 0.5); }

/* message bit j of a frame: n stego bits (one per byte; stego[0] is column `stego_base` of the frame, so that a caller can hand
 * over a staged window), m message bits, invalpha = (double)n / m, the two sub-matrices (shorter = floor, longer = ceil of
 * invalpha).  The guards of the serial extractor -- column < n, reached bit < m -- are kept. */
PCAMV_HD unsigned pcamv_stc_extract_bit(const uint8_t *stego, int stego_base, int n, int m, double invalpha, int shorter, int longer,
                                        const unsigned *cols_short, const unsigned *cols_long, int height, int j)
{
    unsigned acc = 0;
    if (j < 0 || j >= m) return 0;
    for (int i = j - (height - 1) > 0 ? j - (height - 1) : 0; i <= j; i++) {
        const int start = pcamv_stc_before(i, invalpha);
        const int which = (double)(start + longer) <= (i + 1) * invalpha + 0.5, width = which ? longer : shorter;
        const unsigned *cols = which ? cols_long : cols_short;
        const int sh = j - i;
        for (int k = 0; k < width && start + k < n; k++)
            acc ^= (unsigned)stego[start + k - stego_base] & (cols[k] >> sh);
    }
    return acc & 1u;
}

/* first and one-past-last stego column the message bits j0 .. j1 - 1 read */
PCAMV_HD void pcamv_stc_window(int j0, int j1, int n, int m, double invalpha, int height, int *lo, int *hi)
{
    const int i0 = j0 - (height - 1) > 0 ? j0 - (height - 1) : 0, i1 = j1 < m ? j1 : m;
    const int a = pcamv_stc_before(i0, invalpha), b = pcamv_stc_before(i1, invalpha);
    *lo = a < n ? a : n;
    *hi = b < n ? b : n;
}

/* packed payloads: 8 bits per byte, most significant bit first */
PCAMV_HD unsigned pcamv_packed_bit(const uint8_t *bytes, long long i) { return (bytes[i >> 3] >> (7 - (int)(i & 7))) & 1u; }

/* Sub-matrix columns as the embedding and the receiving kernels get them (embed.h:141-199): the published tables for widths 2..20
 * (`table`: pcamv_stc_mats_dev on the device, pcamv_stc_mats on the host; stc_mats.h), columns drawn from the code's own LCG
 * (embed.h:134-139) outside that range; 0, and the generator left where it was, for a width the height has no columns for */
PCAMV_HD int pcamv_stc_matrix(const unsigned *table, int width, int height, unsigned *cols, long long *lcg)
{
    if (width >= 2 && width <= 20 && height >= 7 && height <= 12) {
        for (int i = 0; i < width; i++) cols[i] = table[(height - 7) * 400 + (width - 1) * 20 + i];
        return 1;
    }
    if ((1 << (height - 2)) < width) return 0;
    unsigned mask = (1u << (height - 2)) - 1, bop = (1u << (height - 1)) + 1;
    long hold = (long)*lcg;
    for (int i = 0; i < width; i++) {
        unsigned r = 0; int j;
        for (j = -1; j < i;) {
            hold = (long)((unsigned long)hold * 214013UL + 2531011UL);      /* (the reference's `long` product, wrapping as it does there) */
            r = (((unsigned)(hold >> 16) & 0x7fff & mask) << 1) + bop;
            for (j = 0; j < i; j++) if (cols[j] == r) break;
        }
        cols[i] = r;
    }
    *lcg = hold;
    return 1;
}

/* per-context words of the payload path (device memory; the host check of the receive-side chain keeps the same four) */
enum { PST_TX = 0,            /* payload bits the sender has consumed */
       PST_RX = 1,            /* bits appended to the received stream */
       PST_OVERRUN = 2,       /* != 0: a frame did not fit the reserved received buffer (its tail was dropped, never written) */
       PST_RX_LCG = 3,        /* the receiver's own STC column generator (embed.h:134), started like the sender's */
       PST_WORDS = 4 };

/* What chains from frame to frame on the receiving side, for one frame whose carrier count is known (hdr[0] = n): the frame's m, the
 * two sub-matrices from the receiver's column generator (shorter then longer, as the host extractor calls them), and the frame's
 * place in the received stream.  The write cursor moves by m whatever the frame turns out to be, so that the offsets of sender and
 * receiver stay aligned (m > n, or no matrix for the width: m zero bits -- the stream is zeroed when reserved, so nothing is
 * written for them).  status != 0 (the frame's slice did not parse): no bits, cursor and generator stay, hdr[0] is not read.
 * Thread 64 of k_extract_prepare runs this for its one frame, a lane of k_extract_chain for the slots of a window in slot order.
 * `work` is where the columns are built (the generator compares every new column with all earlier ones: LDS where the caller has
 * some), `cols` where they go once both sub-matrices stand; the two may be the same array.
 * hdr: [0]=n [1]=m [2]=sub-matrices built [6..7]=bit offset of the frame in the received stream, low word first */
/* (the frame itself, whoever decided its place `at`: hdr and the columns, the generator moved; returns m, -1 for status != 0) */
PCAMV_HD int pcamv_extract_chain_frame(const unsigned *table, float emrate, int status, long long at, int *hdr, unsigned *work, unsigned *cols, long long *lcg)
{
    hdr[6] = (int)(unsigned)((unsigned long long)at & 0xffffffffu); hdr[7] = (int)(unsigned)((unsigned long long)at >> 32);
    if (status) { hdr[0] = 0; hdr[1] = 0; hdr[2] = 0; return -1; }
    const int n = hdr[0], m = pcamv_stc_frame_bits(emrate, n);
    const bool sched = m > 0 && m <= n;
    const double invalpha = sched ? (double)n / m : 0.0;
    const int shorter = (int)floor(invalpha), longer = (int)ceil(invalpha);
    const int ok = sched && pcamv_stc_matrix(table, shorter, PCAMV_STC_HEIGHT, work, lcg) && pcamv_stc_matrix(table, longer, PCAMV_STC_HEIGHT, work + STC_MAXW, lcg);
    if (ok && work != cols) {
        for (int k = 0; k < shorter; k++) cols[k] = work[k];
        for (int k = 0; k < longer; k++) cols[STC_MAXW + k] = work[STC_MAXW + k];
    }
    hdr[1] = m; hdr[2] = ok;
    return m;
}
PCAMV_HD void pcamv_extract_chain_slot(const unsigned *table, float emrate, int status, int have_rx, long long rx_cap_bits, int *hdr,
                                       unsigned *work, unsigned *cols, long long *pstate)
{
    const long long at = pstate[PST_RX];
    const int m = pcamv_extract_chain_frame(table, emrate, status, at, hdr, work, cols, pstate + PST_RX_LCG);
    if (m >= 0 && have_rx) {
        pstate[PST_RX] = at + m;
        if (at + m > rx_cap_bits) pstate[PST_OVERRUN] = 1;
    }
}
/* The sibling for a frame whose place was planned for the whole batch (one message for the batch, pcamv_message.h): `at` is given,
 * hdr[6..7] and hdr[1..2] are written and the context's column generator moves as above -- the generators stay per context, advanced in
 * slot order --, while the context's own stream is not involved: PST_RX and PST_OVERRUN stay as they are. */
PCAMV_HD void pcamv_extract_chain_slot_at(const unsigned *table, float emrate, int status, long long at, int *hdr, unsigned *work, unsigned *cols,
                                          long long *pstate)
{
    pcamv_extract_chain_frame(table, emrate, status, at, hdr, work, cols, pstate + PST_RX_LCG);
}

/* host side: the same columns with the widths checked against STC_MAXW (a caller's array) */
static inline int pcamv_stc_matrix_host(const unsigned *table, int width, int height, unsigned *cols, long long *lcg)
{
    if (width >= 2 && width <= 20 && height >= 7 && height <= 12) {
        for (int i = 0; i < width; i++) cols[i] = table[(height - 7) * 400 + (width - 1) * 20 + i];
        return 1;
    }
    if (!lcg || width < 1 || width > STC_MAXW || (1 << (height - 2)) < width) return 0;
    unsigned mask = (1u << (height - 2)) - 1, bop = (1u << (height - 1)) + 1;
    long hold = (long)*lcg;
    for (int i = 0; i < width; i++) {
        unsigned r = 0; int j;
        for (j = -1; j < i;) {
            hold = (long)((unsigned long)hold * 214013UL + 2531011UL);      /* (the reference's `long` product, wrapping as it does there) */
            r = (((unsigned)(hold >> 16) & 0x7fff & mask) << 1) + bop;
            for (j = 0; j < i; j++) if (cols[j] == r) break;
        }
        cols[i] = r;
    }
    *lcg = hold;
    return 1;
}
#endif
