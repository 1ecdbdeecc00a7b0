/*
 * pcamv_source.hip.h -- the source feed (gfx950), launched by pcamv_gpu.hip only; the control code is pcamv_source.h.
 *
 *   k_source_feed   one wavefront per (context, work item): the context's next picture out of the caller's clip into its own source
 *                   planes, padded to whole macroblocks.  Bandwidth and nothing else: ordinary vector loads, as wide as the source
 *                   address allows, and 16-byte stores (8 in chroma rows of an odd mb_w) over contiguous spans of the tight planes;
 *                   no LDS, no atomics, no wave waits for another -- the item that holds the last real row reads it again for
 *                   the rows of padding below it.
 */
#ifndef PCAMV_SOURCE_HIP_H
#define PCAMV_SOURCE_HIP_H
#include "pcamv_source.h"

struct SrcFeed {
    pcamv_source_t S;
    const uint8_t *clip;
    const long long *picture;       /* [n] the caller's indices */
    uint8_t *const *planes;         /* [n][3] the contexts' source planes */
    int *status;                    /* [n] */
    long long n_pictures;           /* whole pictures in the clip (src_check) */
    int mb_w, mb_h, n;
};

static __global__ void __launch_bounds__(64) k_source_feed(const SrcFeed J)
{
    const int items = src_items(J.mb_h);
    const int ctx = (int)(blockIdx.x / (unsigned)items), item = (int)(blockIdx.x % (unsigned)items), lane = threadIdx.x;
    if (ctx >= J.n) return;
    const long long pic = J.picture[ctx];
    const bool ok = pic >= 0 && pic < J.n_pictures;
    if (item == 0 && lane == 0) J.status[ctx] = ok ? 0 : PCAMV_EINVAL;
    if (!ok) return;                /* an index outside the clip: nothing of the context's planes is written */
    uint8_t *const dst[3] = {J.planes[3 * ctx], J.planes[3 * ctx + 1], J.planes[3 * ctx + 2]};
    src_item_lane(&J.S, J.clip + pic * J.S.picture_stride, dst, J.mb_w, J.mb_h, item, lane);
}
#endif
