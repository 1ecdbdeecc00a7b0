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
/* Every kernel is batched over independent closed GOPs: blockIdx.z (plane kernels) or blockIdx.y
 * (macroblock kernels) selects the GOP's FrameDev in a device array.  One launch then carries
 * the same dependency step of all GOPs, which is what fills the 256 CUs (a single 1080p frame
 * exposes at most 60 independent macroblocks at a time). */
static __global__ void __launch_bounds__(256) k_chroma_pad(const FrameDev *__restrict__ Fs)
{
    const FrameDev &F = Fs[blockIdx.z >> 1];
    const int pl = blockIdx.z & 1;
    const uint8_t *__restrict__ src = F.raw[1 + pl];
    uint8_t *__restrict__ dst = F.chroma_base[pl];
    const int w = F.w >> 1, h = F.h >> 1, cstride = F.cstride, clines = F.clines;
    /* 4 pixels per thread; pad and width are multiples of 4, so a group is inside the picture or one replicated pixel */
    const int x = 4 * (blockIdx.x * blockDim.x + threadIdx.x), y = blockIdx.y;
    if (x >= cstride || y >= clines) return;
    const uint8_t *rowp = src + (size_t)clip3i(y - PCAMV_CPAD, 0, h - 1) * w;
    const int gx = x - PCAMV_CPAD;
    uint32_t v;
    if (gx < 0 || gx >= w) v = rowp[gx < 0 ? 0 : w - 1] * 0x01010101u;
    else if (((uintptr_t)src & 3) == 0) v = *(const uint32_t *)(rowp + gx);
    else v = rowp[gx] | rowp[gx + 1] << 8 | rowp[gx + 2] << 16 | (uint32_t)rowp[gx + 3] << 24;
    *(uint32_t *)(dst + (size_t)y * cstride + x) = v;
}

/* (clamp_u8: pcamv_prims_gpu.h) */
/* The four luma planes full / H / V / HV of the reference frame, padded (x264_frame_filter + expand_border,
 * common/mc.c:455-507, frame.c:246-300; the filtered planes are defined 4 columns / 8 rows beyond the picture and
 * replicated from there).  One thread = 4 horizontally adjacent output pixels, walking HP_ROWS rows down: it keeps
 * the 6 source rows x 12 source columns its filters need in registers (three dwords a row, one new row per output
 * row), so a source byte is fetched once per thread and never goes through LDS; every store is a full dword and a
 * wave's stores are contiguous.  The output pixel groups are aligned with the picture (pad and width are multiples
 * of 4), so a group is either inside the filtered domain or entirely replicated from its edge pixel. */
#define HP_ROWS 16
#define HP_THREADS 128
__device__ __forceinline__ void hpel_load_row(const uint8_t *__restrict__ rowp, int eg0, int W, bool fast, uint32_t d[3])
{
    if (fast) {
        const uint32_t *q = (const uint32_t *)(rowp + eg0 - 4);
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
    const FrameDev &F = Fs[blockIdx.z];
    const uint8_t *__restrict__ src = F.raw[0];
    uint8_t *__restrict__ planes = F.luma_base;
    const int W = F.w, H = F.h, stride = F.stride, lines = F.lines;
    const int x0 = 4 * (blockIdx.x * HP_THREADS + threadIdx.x), yb = blockIdx.y * HP_ROWS;
    if (x0 >= stride) return;
    /* first picture column of the group whose values this group shows, and which of its bytes when replicated */
    const int gx = x0 - PCAMV_PAD, eg0 = clip3i(gx, -4, W);
    const int rep = gx < -4 ? 0 : gx > W ? 3 : -1;
    const bool fast = eg0 >= 4 && eg0 + 8 <= W && ((uintptr_t)src & 3) == 0;
    const size_t psz = (size_t)F.plane_size;
    const unsigned strip = PCAMV_LSTRIP_OF(x0);
    const size_t strip_o = (size_t)x0 + (size_t)strip * (size_t)F.lskip;
    const bool dup = strip > 0 && (unsigned)x0 == strip * PCAMV_LSW;
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
        /* strip layout (pcamv_common.h): the group's place in its own strip and, for a strip's first group, the repeat at the end
         * of the strip before it */
        const size_t o = (size_t)y * PCAMV_LROW + strip_o;
        *(uint32_t *)(planes + o) = of;
        if (F.luma_raster) *(uint32_t *)(F.luma_raster + (size_t)y * stride + x0) = of;
        *(uint32_t *)(planes + psz + o) = oh;
        *(uint32_t *)(planes + 2 * psz + o) = ov;
        *(uint32_t *)(planes + 3 * psz + o) = oc;
        if (dup) {
            const size_t o2 = o - (size_t)F.lskip;
            *(uint32_t *)(planes + o2) = of;
            *(uint32_t *)(planes + psz + o2) = oh;
            *(uint32_t *)(planes + 2 * psz + o2) = ov;
            *(uint32_t *)(planes + 3 * psz + o2) = oc;
        }
    }
}
#endif
