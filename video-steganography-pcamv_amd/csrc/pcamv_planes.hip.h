/*
 * pcamv_planes.hip.h -- plane production (gfx950), launched by pcamv_gpu.hip only.
 *
 *   k_chroma_pad      reference chroma -> padded planes (x264_frame_expand_border, frame.c:246)
 *   k_hpel            reference luma -> 4 padded planes full/H/V/HV in the strip layout of pcamv_common.h, 6-tap filter with
 *                     the source window in registers (hpel_filter mc.c:167-190 + both border expansions, frame.c:246-301, in
 *                     closed form: value(x,y) = filter(clamp(x,-4,W+3), clamp(y,-8,H+7)))
 */
#ifndef PCAMV_PLANES_HIP_H
#define PCAMV_PLANES_HIP_H
#include "pcamv_common.h"
#include "pcamv_prims_gpu.h"

/* ------------------------------------------------------------------ plane production */
/* stores go out as global_store (address space 1), not flat: 16 bytes a lane, whole 128-byte lines a wave */
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 *gp128w;
typedef __attribute__((address_space(1))) uint32_t *gp32w;
typedef const __attribute__((address_space(1))) uint32_t *gp32;
/* Every kernel is batched over independent closed GOPs: blockIdx.z (plane kernels) or blockIdx.y
 * (macroblock kernels) selects the GOP's FrameDev in a device array.  One launch then carries
 * the same dependency step of all GOPs, which is what fills the 256 CUs (a single 1080p frame
 * exposes at most 60 independent macroblocks at a time). */
/* One thread = 16 horizontally adjacent bytes of a padded chroma row (cstride is a multiple of 16; the pad and the width are
 * multiples of 4, so each of the four dwords is inside the picture or one replicated pixel), CP_ROWS rows per block: a wave's store
 * instruction covers whole 128-byte lines. */
#define CP_ROWS 4
#define CP_THREADS 256
static __global__ void __launch_bounds__(CP_THREADS) k_chroma_pad(const FrameDev *__restrict__ Fs)
{
    const FrameDev &F = Fs[blockIdx.z >> 1];
    const int pl = blockIdx.z & 1;
    const uint8_t *__restrict__ src = F.raw[1 + pl];
    uint8_t *__restrict__ dst = F.chroma_base[pl];
    const int w = F.w >> 1, h = F.h >> 1, cstride = F.cstride, clines = F.clines;
    const int per_row = cstride >> 4;                        /* threads a row takes */
    const int i = blockIdx.x * CP_THREADS + threadIdx.x;
    const int y = blockIdx.y * CP_ROWS + i / per_row, x = 16 * (i % per_row);
    if (i >= per_row * CP_ROWS || y >= clines) return;
    const uint8_t *rowp = src + (size_t)clip3i(y - PCAMV_CPAD, 0, h - 1) * w;
    const bool aligned = ((uintptr_t)src & 3) == 0;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int gx = x + 4 * k - PCAMV_CPAD;
        if (gx < 0 || gx >= w) v[k] = rowp[gx < 0 ? 0 : w - 1] * 0x01010101u;
        else if (aligned) v[k] = *(const uint32_t *)(rowp + gx);
        else v[k] = rowp[gx] | rowp[gx + 1] << 8 | rowp[gx + 2] << 16 | (uint32_t)rowp[gx + 3] << 24;
    }
    *(gp128w)(dst + (size_t)y * cstride + x) = u32x4{v[0], v[1], v[2], v[3]};
}

/* (clamp_u8: pcamv_prims_gpu.h) */
/* The four luma planes full / H / V / HV of the reference frame, padded (x264_frame_filter + expand_border,
 * common/mc.c:455-507, frame.c:246-300; the filtered planes are defined 4 columns / 8 rows beyond the picture and
 * replicated from there).  One thread = one dword of a strip (pcamv_common.h): 4 horizontally adjacent output pixels
 * of the padded columns 28 s + 4 d .. + 3, d = 0 .. 7, walking HP_ROWS rows down.  It keeps the 6 source rows x 12
 * source columns its filters need in registers (three dwords a row, one new row per output row), so a source byte is
 * fetched once per thread.  A strip's last dword (d = 7) shows the same columns as the next strip's first: it is an
 * output group like any other (the filter is closed-form in x), there is no second store.  The output pixel groups are
 * aligned with the picture (pad, width and 28 are multiples of 4), so a group is either inside the filtered domain or
 * entirely replicated from its edge pixel.
 * Stores: a 128-byte line of the layout is rows 4 q .. 4 q + 3 of one strip.  A wave (8 strips x 8 dwords) parks four
 * finished rows of the four planes in LDS (4 planes x 8 strips x 128 bytes, the strips HP_TILE dwords apart so that
 * the 64 lanes of a row write hit 64 banks), then every lane takes 16 bytes of its own strip's line back and the
 * wave's global_store_dwordx4 covers eight whole lines per plane. */
#define HP_ROWS 16
#define HP_THREADS 64
#define HP_TILE 40
__device__ __forceinline__ void hpel_load_row(const uint8_t *__restrict__ rowp, int eg0, int W, bool fast, uint32_t d[3])
{
    if (fast) {
        const gp32 q = (gp32)(rowp + eg0 - 4);
        d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) v |= (uint32_t)rowp[clip3i(eg0 - 4 + 4 * i + b, 0, W - 1)] << (8 * b);
            d[i] = v;
        }
    }
}
static __global__ void __launch_bounds__(HP_THREADS) k_hpel(const FrameDev *__restrict__ Fs)
{
    __shared__ uint32_t tile[4][8][HP_TILE];
    const FrameDev &F = Fs[blockIdx.z];
    const uint8_t *__restrict__ src = F.raw[0];
    uint8_t *__restrict__ planes = F.luma_base;
    const int W = F.w, H = F.h, stride = F.stride, lines = F.lines;
    const int t = threadIdx.x >> 3, d = threadIdx.x & 7;
    const int strip = blockIdx.x * 8 + t, yb = blockIdx.y * HP_ROWS;
    if (strip * PCAMV_LSW >= stride) return;             /* (strips that begin beyond the stride are never read) */
    const int x0 = strip * PCAMV_LSW + 4 * d;
    /* first picture column of the group whose values this group shows, and which of its bytes when replicated */
    const int gx = x0 - PCAMV_PAD, eg0 = clip3i(gx, -4, W);
    const int rep = gx < -4 ? 0 : gx > W ? 3 : -1;
    const bool fast = eg0 >= 4 && eg0 + 8 <= W && ((uintptr_t)src & 3) == 0;
    const size_t psz = (size_t)F.plane_size;
    /* the lane's 16 bytes of its strip's line: row d / 2 of the four, half d % 2 */
    uint8_t *const line0 = planes + (size_t)strip * PCAMV_LROW * (size_t)lines + 16 * d;
    const bool raster = F.luma_raster && d < 7 && x0 < stride;
    uint32_t w[6][3];
    uint32_t of = 0, oh = 0, ov = 0, oc = 0;
    int ey_prev = 0;
    for (int y = yb; y < yb + HP_ROWS && y < lines; y++) {
        const int ey = clip3i(y - PCAMV_PAD, -8, H + 7);
        if (y == yb || ey != ey_prev) {
            if (y == yb) {
#pragma unroll
                for (int k = 0; k < 5; k++) hpel_load_row(src + (size_t)clip3i(ey - 2 + k, 0, H - 1) * W, eg0, W, fast, w[k]);
            } else {
#pragma unroll
                for (int k = 0; k < 5; k++) { w[k][0] = w[k + 1][0]; w[k][1] = w[k + 1][1]; w[k][2] = w[k + 1][2]; }
            }
            hpel_load_row(src + (size_t)clip3i(ey + 3, 0, H - 1) * W, eg0, W, fast, w[5]);
            ey_prev = ey;
            /* window positions 2..10 = picture columns eg0-2 .. eg0+6: unrounded vertical 6-tap of each, and row 2 itself */
            int v[9], b2[9];
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const int q = (j + 2) >> 2, sh = 8 * ((j + 2) & 3);
#define HPB(k) ((int)(w[k][q] >> sh & 255))
                v[j] = HPB(0) + HPB(5) - 5 * (HPB(1) + HPB(4)) + 20 * (HPB(2) + HPB(3));
                b2[j] = HPB(2);
#undef HPB
            }
            of = w[2][1]; oh = ov = oc = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int th = b2[k] + b2[k + 5] - 5 * (b2[k + 1] + b2[k + 4]) + 20 * (b2[k + 2] + b2[k + 3]);
                const int tc = v[k] + v[k + 5] - 5 * (v[k + 1] + v[k + 4]) + 20 * (v[k + 2] + v[k + 3]);
                oh |= clamp_u8((th + 16) >> 5) << (8 * k);
                ov |= clamp_u8((v[k + 2] + 16) >> 5) << (8 * k);
                oc |= clamp_u8((tc + 512) >> 10) << (8 * k);
            }
            if (rep >= 0) {
                const int sh = 8 * rep;
                of = (of >> sh & 255) * 0x01010101u; oh = (oh >> sh & 255) * 0x01010101u;
                ov = (ov >> sh & 255) * 0x01010101u; oc = (oc >> sh & 255) * 0x01010101u;
            }
        }
        if (raster) *(gp32w)(F.luma_raster + (size_t)y * stride + x0) = of;
        /* (yb and lines are multiples of 4: a walk is made of whole lines) */
        const int r = y & 3;
        tile[0][t][8 * r + d] = of; tile[1][t][8 * r + d] = oh; tile[2][t][8 * r + d] = ov; tile[3][t][8 * r + d] = oc;
        if (r == 3) {
            PCAMV_WAVE_SYNC();
            u32x4 ln[4];
#pragma unroll
            for (int k = 0; k < 4; k++) ln[k] = *(const u32x4 *)&tile[k][t][4 * d];
            PCAMV_WAVE_SYNC();
            uint8_t *const o = line0 + (size_t)(y - 3) * PCAMV_LROW;
#pragma unroll
            for (int k = 0; k < 4; k++) *(gp128w)(o + k * psz) = ln[k];
        }
    }
}
#endif
