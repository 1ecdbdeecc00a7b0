/*
 * stc_extract_driver.cpp -- TEST-ONLY host build of the receiver's per-message-bit function (csrc/pcamv_stc_extract.h), the code
 * k_extract_bits runs one thread per bit of.  Lets `pytest -m "not gpu"` compare it with the library's serial extractor and the
 * oracle's, without a GPU.  It is NOT a fallback: libpcamv_gpu.so never links it.
 */
#include <stdlib.h>
#include <string.h>
#include "stc_mats.h"
#include "pcamv_stc_extract.h"

extern "C" int stcx_frame_bits(float emrate, int n) { return pcamv_stc_frame_bits(emrate, n); }

/* a frame the way the two kernels take it: both sub-matrices (shorter, then longer) from the generator state *lcg, then every
 * message bit on its own.  window > 0: the bits in groups of `window`, each group reading a copy of exactly the stego columns
 * pcamv_stc_window names (what a workgroup stages through LDS; the copy is heap memory of that size, for the sanitizers). */
extern "C" int stcx_extract(const uint8_t *stego, int n, int m, int height, long long *lcg, int window, uint8_t *message)
{
    if (!stego || !message || !lcg || n <= 0 || m <= 0 || m > n) return -1;
    const double invalpha = (double)n / m;
    const int shorter = (int)floor(invalpha), longer = (int)ceil(invalpha);
    unsigned cs[STC_MAXW], cl[STC_MAXW];
    if (longer > STC_MAXW || !pcamv_stc_matrix_host(pcamv_stc_mats, shorter, height, cs, lcg) || !pcamv_stc_matrix_host(pcamv_stc_mats, longer, height, cl, lcg)) return -5;
    if (window <= 0) {
        for (int j = 0; j < m; j++) message[j] = (uint8_t)pcamv_stc_extract_bit(stego, 0, n, m, invalpha, shorter, longer, cs, cl, height, j);
        return 0;
    }
    for (int j0 = 0; j0 < m; j0 += window) {
        int lo, hi;
        pcamv_stc_window(j0, j0 + window, n, m, invalpha, height, &lo, &hi);
        if (lo < 0 || hi > n || hi < lo) return -2;
        uint8_t *win = (uint8_t *)malloc(hi - lo > 0 ? hi - lo : 1);
        if (!win) return -3;
        memcpy(win, stego + lo, hi - lo);
        for (int j = j0; j < j0 + window && j < m; j++) message[j] = (uint8_t)pcamv_stc_extract_bit(win, lo, n, m, invalpha, shorter, longer, cs, cl, height, j);
        free(win);
    }
    return 0;
}
