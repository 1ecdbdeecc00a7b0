/*
 * pcamv_source.h -- the sender's source pictures: a picture of any even size out of a caller's clip (planar or semi-planar 4:2:0, any
 * pitch, any alignment, top-down or bottom-up) into the three tightly packed planes of the coded size, padded to whole macroblocks.
 * The control code of k_source_feed (pcamv_source.hip.h), and the definition it is held to.
 *
 * Compiles for the device, for the host side of the library (pcamv_gpu_source_picture, pcamv_gpu_source_check: the definition without
 * a GPU) and for plain C++ test programs (tests/fuzz/check_source.cpp, with PCAMV_HOST_EMU): no HIP type, no table in memory.
 *
 * The rule restates x264_frame_copy_picture (common/frame.c:190-220: YV12 swaps planes 1 and 2, VFLIP reads the lines bottom-up)
 * followed by x264_frame_expand_border_mod16 (common/frame.c:310-337: the last real sample of a line repeated to the right, then the
 * last real line repeated downwards): coded plane i, W_i x H_i = (16 mb_w >> !!i) x (16 mb_h >> !!i), holds
 *     out_i[y][x] = src_i[min(y, h_i - 1)][min(x, w_i - 1)],   w_i = width >> !!i, h_i = height >> !!i.
 * NV12 / NV21 (not the reference's: what decoders and capture paths hand out) take the two chroma planes from the even and the odd
 * bytes of plane 1.
 *
 * src_picture_naive is the definition: sequential, a sample at a time.  src_item_lane is the kernel's: a work item is one macroblock
 * row of luma (items 0 .. mb_h - 1) or of both chroma planes (items mb_h .. 2 mb_h - 1); the item's destination bytes are one
 * contiguous span of the tight plane, cut into chunks of 16 bytes (8 in chroma rows of an odd mb_w, which are only 8-byte aligned),
 * chunk k the k-th lane's in rounds of 64: a wavefront's store covers whole 128-byte lines wherever the span has them.  Each chunk is
 * loaded with the widest loads its source address allows (16, 8, 4, 2, 1 bytes), byte by byte where it crosses the picture's right
 * edge, and reads no byte outside the picture's own samples.
 */
#ifndef PCAMV_SOURCE_H
#define PCAMV_SOURCE_H
#include <stddef.h>
#include <stdint.h>
#include "pcamv_common.h"

#if defined(__HIPCC__) && !defined(PCAMV_HOST_EMU)
#define PCAMV_SRC_HD __host__ __device__ static inline
#else
#define PCAMV_SRC_HD static inline
#endif

#define SRC_DIM_MAX 65536               /* macroblocks per side, as the SPS allows */
#define SRC_BYTES_MAX (1LL << 40)       /* offsets, pitches and the distance between pictures: their products with a height stay inside int64 */

/* where coded plane i comes from: the caller's plane, the first byte's offset in it, and the bytes between samples */
struct SrcPlane { int plane, first, step; };
PCAMV_SRC_HD SrcPlane src_plane(int format, int i)
{
    SrcPlane p = {i, 0, 1};
    if (i && format == PCAMV_SRC_YV12) p.plane = i ^ 3;
    if (i && (format == PCAMV_SRC_NV12 || format == PCAMV_SRC_NV21)) { p.plane = 1; p.step = 2; p.first = (i == 2) ^ (format == PCAMV_SRC_NV21); }
    return p;
}
PCAMV_SRC_HD int src_semiplanar(int format) { return format == PCAMV_SRC_NV12 || format == PCAMV_SRC_NV21; }

/* pcamv_gpu_source_check */
PCAMV_SRC_HD int src_check(const pcamv_source_t *S, long long clip_bytes, int mb_w, int mb_h, long long *n_pictures)
{
    if (n_pictures) *n_pictures = 0;
    if (!S || clip_bytes < 0 || mb_w < 1 || mb_w > SRC_DIM_MAX || mb_h < 1 || mb_h > SRC_DIM_MAX) return PCAMV_EINVAL;
    if (S->width < 2 || S->height < 2 || (S->width & 1) || (S->height & 1)) return PCAMV_EINVAL;
    if (S->width <= 16 * (mb_w - 1) || S->width > 16 * mb_w || S->height <= 16 * (mb_h - 1) || S->height > 16 * mb_h) return PCAMV_EINVAL;
    if (S->format != PCAMV_SRC_I420 && S->format != PCAMV_SRC_YV12 && S->format != PCAMV_SRC_NV12 && S->format != PCAMV_SRC_NV21) return PCAMV_EINVAL;
    if (S->flags & ~PCAMV_SRC_VFLIP) return PCAMV_EINVAL;
    if (S->picture_stride < 1 || S->picture_stride > SRC_BYTES_MAX) return PCAMV_EINVAL;
    const int planes = src_semiplanar(S->format) ? 2 : 3;
    long long extent = 0;               /* the bytes of a picture, from its start to the end of its last sample */
    for (int k = 0; k < planes; k++) {
        const long long line = k == 0 || planes == 2 ? S->width : S->width / 2, lines = S->height >> !!k;
        if (S->plane_off[k] < 0 || S->plane_off[k] > SRC_BYTES_MAX || S->pitch[k] < line || S->pitch[k] > SRC_BYTES_MAX) return PCAMV_EINVAL;
        const long long end = S->plane_off[k] + (lines - 1) * S->pitch[k] + line;
        if (end > extent) extent = end;
    }
    if (n_pictures && clip_bytes >= extent) *n_pictures = (clip_bytes - extent) / S->picture_stride + 1;
    return 0;
}

/* the definition.  pic: the picture's first byte; out: three tight planes of the coded size */
static inline void src_picture_naive(const pcamv_source_t *S, const uint8_t *pic, int mb_w, int mb_h, uint8_t *const out[3])
{
    for (int i = 0; i < 3; i++) {
        const SrcPlane P = src_plane(S->format, i);
        const int W = 16 * mb_w >> !!i, H = 16 * mb_h >> !!i, w = S->width >> !!i, h = S->height >> !!i;
        const uint8_t *base = pic + S->plane_off[P.plane] + P.first;
        for (int y = 0; y < H; y++) {
            const int sy = y < h ? y : h - 1;
            const uint8_t *line = base + (long long)((S->flags & PCAMV_SRC_VFLIP) ? h - 1 - sy : sy) * S->pitch[P.plane];
            for (int x = 0; x < W; x++) out[i][(size_t)y * W + x] = line[(x < w ? x : w - 1) * P.step];
        }
    }
}

/* ---- the kernel's control code */
struct alignas(16) SrcV16 { uint32_t w[4]; };
struct alignas(8) SrcV8 { uint32_t w[2]; };
#if defined(__HIPCC__) && !defined(PCAMV_HOST_EMU)
#define SRC_UNROLL _Pragma("unroll")
#else
#define SRC_UNROLL
#endif

/* N bytes (a multiple of 8) at p into N / 4 dwords, by the widest loads p's alignment allows; the classes a census counts: 0 .. 4 for
 * 16, 8, 4, 2, 1 */
PCAMV_SRC_HD int src_align_class(const uint8_t *p) { const uintptr_t a = (uintptr_t)p; return !(a & 15) ? 0 : !(a & 7) ? 1 : !(a & 3) ? 2 : !(a & 1) ? 3 : 4; }
template <int N> PCAMV_SRC_HD void src_load(const uint8_t *p, uint32_t *w)
{
    const uintptr_t a = (uintptr_t)p;
    if (N % 16 == 0 && !(a & 15)) {
        SRC_UNROLL for (int k = 0; k < N / 16; k++) { const SrcV16 v = ((const SrcV16 *)(const void *)p)[k]; w[4 * k] = v.w[0]; w[4 * k + 1] = v.w[1]; w[4 * k + 2] = v.w[2]; w[4 * k + 3] = v.w[3]; }
    } else if (!(a & 7)) {
        SRC_UNROLL for (int k = 0; k < N / 8; k++) { const SrcV8 v = ((const SrcV8 *)(const void *)p)[k]; w[2 * k] = v.w[0]; w[2 * k + 1] = v.w[1]; }
    } else if (!(a & 3)) {
        SRC_UNROLL for (int k = 0; k < N / 4; k++) w[k] = ((const uint32_t *)(const void *)p)[k];
    } else if (!(a & 1)) {
        SRC_UNROLL for (int k = 0; k < N / 4; k++) { const uint16_t *q = (const uint16_t *)(const void *)p; w[k] = (uint32_t)q[2 * k] | (uint32_t)q[2 * k + 1] << 16; }
    } else {
        SRC_UNROLL for (int k = 0; k < N / 4; k++) w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
    }
}
/* a chunk that crosses the right edge: CB samples `step` bytes apart of which `valid` (1 .. CB - 1) exist; the last one repeats */
template <int CB> PCAMV_SRC_HD void src_load_edge(const uint8_t *p, int step, int valid, uint32_t *w)
{
    SRC_UNROLL for (int k = 0; k < CB / 4; k++) {
        uint32_t v = 0;
        SRC_UNROLL for (int j = 0; j < 4; j++) { const int x = 4 * k + j; v |= (uint32_t)p[(x < valid ? x : valid - 1) * step] << (8 * j); }
        w[k] = v;
    }
}
/* the even bytes of the 8 bytes {lo, hi} (odd = 0), or the odd ones (odd = 1) */
PCAMV_SRC_HD uint32_t src_split(uint32_t lo, uint32_t hi, int odd)
{
    lo >>= 8 * odd; hi >>= 8 * odd;
    return (lo & 0xff) | (lo >> 8 & 0xff00) | (hi & 0xff) << 16 | (hi >> 8 & 0xff00) << 16;
}
template <int CB> PCAMV_SRC_HD void src_store(uint8_t *dst, const uint32_t *w)
{
    if (CB == 16) { SrcV16 v; v.w[0] = w[0]; v.w[1] = w[1]; v.w[2] = w[2]; v.w[3] = w[3]; *(SrcV16 *)(void *)dst = v; }
    else { SrcV8 v; v.w[0] = w[0]; v.w[1] = w[1]; *(SrcV8 *)(void *)dst = v; }
}

/* rows [y0, y0 + rows) of one coded plane of width W (a multiple of CB) from a plane of single samples, w x h: lane's chunks */
template <int CB> PCAMV_SRC_HD void src_rows_planar(const uint8_t *src, long long pitch, int w, int h, int flip, uint8_t *dst, int W, int y0, int rows, int lane)
{
    const unsigned C = (unsigned)(W / CB), total = (unsigned)rows * C;
    for (unsigned k = (unsigned)lane; k < total; k += 64) {
        const unsigned r = k / C, c = k - r * C;
        const int y = y0 + (int)r, sy = y < h ? y : h - 1, x = (int)c * CB;
        const uint8_t *p = src + (long long)(flip ? h - 1 - sy : sy) * pitch + x;
        uint32_t v[CB / 4];
        if (w - x >= CB) src_load<CB>(p, v);
        else src_load_edge<CB>(p, 1, w - x, v);
        src_store<CB>(dst + (size_t)y * (size_t)W + (size_t)x, v);
    }
}
/* the same rows of both chroma planes from one plane of sample pairs; first: which byte of a pair goes to dst_a (the other to dst_b) */
template <int CB> PCAMV_SRC_HD void src_rows_pairs(const uint8_t *src, long long pitch, int w, int h, int flip, int first, uint8_t *dst_a, uint8_t *dst_b, int W, int y0, int rows, int lane)
{
    const unsigned C = (unsigned)(W / CB), total = (unsigned)rows * C;
    for (unsigned k = (unsigned)lane; k < total; k += 64) {
        const unsigned r = k / C, c = k - r * C;
        const int y = y0 + (int)r, sy = y < h ? y : h - 1, x = (int)c * CB;
        const uint8_t *p = src + (long long)(flip ? h - 1 - sy : sy) * pitch + 2 * x;
        uint32_t a[CB / 4], b[CB / 4];
        if (w - x >= CB) {
            uint32_t v[CB / 2];
            src_load<2 * CB>(p, v);
            SRC_UNROLL for (int j = 0; j < CB / 4; j++) { a[j] = src_split(v[2 * j], v[2 * j + 1], first); b[j] = src_split(v[2 * j], v[2 * j + 1], first ^ 1); }
        } else { src_load_edge<CB>(p + first, 2, w - x, a); src_load_edge<CB>(p + (first ^ 1), 2, w - x, b); }
        const size_t at = (size_t)y * (size_t)W + (size_t)x;
        src_store<CB>(dst_a + at, a); src_store<CB>(dst_b + at, b);
    }
}
template <int CB> PCAMV_SRC_HD void src_item_chroma(const pcamv_source_t *S, const uint8_t *pic, uint8_t *const dst[3], int mb_w, int row, int lane)
{
    const int W = 8 * mb_w, w = S->width >> 1, h = S->height >> 1, flip = S->flags & PCAMV_SRC_VFLIP;
    if (src_semiplanar(S->format))
        src_rows_pairs<CB>(pic + S->plane_off[1], S->pitch[1], w, h, flip, S->format == PCAMV_SRC_NV21, dst[1], dst[2], W, 8 * row, 8, lane);
    else
        for (int i = 1; i < 3; i++) {
            const SrcPlane P = src_plane(S->format, i);
            src_rows_planar<CB>(pic + S->plane_off[P.plane], S->pitch[P.plane], w, h, flip, dst[i], W, 8 * row, 8, lane);
        }
}
/* lane's share of work item `item` of a picture (S checked by src_check against mb_w x mb_h; dst: 16-byte aligned tight planes) */
PCAMV_SRC_HD void src_item_lane(const pcamv_source_t *S, const uint8_t *pic, uint8_t *const dst[3], int mb_w, int mb_h, int item, int lane)
{
    if (item < mb_h) src_rows_planar<16>(pic + S->plane_off[0], S->pitch[0], S->width, S->height, S->flags & PCAMV_SRC_VFLIP, dst[0], 16 * mb_w, 16 * item, 16, lane);
    else if (mb_w & 1) src_item_chroma<8>(S, pic, dst, mb_w, item - mb_h, lane);
    else src_item_chroma<16>(S, pic, dst, mb_w, item - mb_h, lane);
}
PCAMV_SRC_HD int src_items(int mb_h) { return 2 * mb_h; }
#endif
