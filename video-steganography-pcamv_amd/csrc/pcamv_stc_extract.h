/*
 * pcamv_stc_extract.h -- the receiving side of the syndrome-trellis code, one message bit at a time.
 *
 * Compiles for the device (k_extract_prepare / k_extract_bits, and the message length k_embed_prepare shares with them), for the host
 * side of the library (the column generator of pcamv_gpu_stc_extract_lcg) and for a plain C++ test driver
 * (tests/emu/stc_extract_driver.cpp): no HIP type, no table of its own.
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

/* host side: sub-matrix columns as the embedder gets them (embed.h:141-199): the published tables for widths 2..20 (`table` = pcamv_stc_mats,
 * stc_mats.h), columns drawn from the code's own LCG (embed.h:134-139) outside that range */
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
            hold = hold * 214013L + 2531011L;
            r = (((unsigned)(hold >> 16) & 0x7fff & mask) << 1) + bop;
            for (j = 0; j < i; j++) if (cols[j] == r) break;
        }
        cols[i] = r;
    }
    *lcg = hold;
    return 1;
}
#endif
